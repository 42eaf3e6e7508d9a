/*
 * fqtk_match.h -- C ABI of the MI355X-native sample-barcode matcher (libfqtk_match.so).
 *
 * This is the drop-in boundary for the ONE hot path of `fqtk demux`: the reference's
 * `BarcodeMatcher` (reference: /root/reference/src/lib/barcode_matching.rs).  The reference has no
 * FFI of its own; each entry point below names the Rust item it replaces so a maintainer can bind it
 * from Rust (`extern "C"`), C++ or ctypes.  Plain pointers and sizes only.
 *
 * Semantics every entry point implements, bit for bit:
 *   enc(b):  'N','n','.' -> 0xF; else IUPAC mask of the upper-cased byte (A1 C2 G4 T8 U8 M3 R5 W9 S6
 *            Y10 K12 V7 H11 D13 B14 N15); any other byte -> 0            (src/lib/mod.rs:26-61)
 *   mm[s]  = #{ i < L : enc(read[i]) & ~enc(barcode_s[i]) != 0 }          (src/lib/bitenc.rs:432-459)
 *   best   = min_s mm[s]; idx = LOWEST s attaining it; next = second smallest with multiplicity
 *            (255 when there is one sample)                      (barcode_matching.rs:119-160)
 *   None   when len < L, when best > max_mismatches, or when next - best < min_mismatch_delta
 *                                                                 (barcode_matching.rs:150-186)
 *   error  when len > L and the no-call prefilter (barcode_matching.rs:170-172) does not reject the
 *            read first -- the reference panics there (barcode_matching.rs:95-107) -> FQTK_ELEN.
 *
 * There is NO CPU fallback behind this ABI: every compute entry point needs a gfx950 device and
 * returns FQTK_ENODEV / FQTK_EHIP otherwise.
 *
 * Threading: a handle is not thread-safe (the reference's matcher is `&mut self`); use one handle per
 * (device, host thread).  Batches on one handle complete in submission order.
 */
#ifndef FQTK_MATCH_H
#define FQTK_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference aborts with panic!/assert!; nothing here aborts) ------------ */
#define FQTK_OK 0
#define FQTK_EINVAL 1 /* bad argument / table precondition (barcode_matching.rs:61-65, samples.rs:101-133) */
#define FQTK_ELEN 2   /* observed barcode longer than expected: the reference's panic (barcode_matching.rs:95-107) */
#define FQTK_EHIP 3   /* a HIP runtime call failed; see fqtk_last_error() */
#define FQTK_ENOMEM 4
#define FQTK_ENODEV 5 /* no usable gfx950 device */
#define FQTK_ENCCL 6  /* RCCL could not be loaded or a collective failed (fqtk_matchers_allreduce_counts) */

#define FQTK_NO_MATCH 0xFFFFu /* fqtk_match_t.idx of a read the reference assigns None */
#define FQTK_MAX_BARCODE_LEN 128u
#define FQTK_MAX_SAMPLES 65534u

/* Replaces `BarcodeMatch { best_match: usize, best_mismatches: u8, next_best_mismatches: u8 }`
 * (barcode_matching.rs:16-25) / `Option<BarcodeMatch>`.  idx == FQTK_NO_MATCH <=> None; then best and
 * next are both 255 (the reference exposes no values for None). 4 bytes, little-endian. */
typedef struct fqtk_match_t {
    uint16_t idx;
    uint8_t best;
    uint8_t next;
} fqtk_match_t;

/* Opaque; owns the device-resident expected-barcode table, error word and staging buffers.
 * Replaces `struct BarcodeMatcher` (barcode_matching.rs:29-45). */
typedef struct fqtk_matcher fqtk_matcher;

/* Thread-local message of the last non-OK status returned on this thread. */
const char *fqtk_last_error(void);

/* ABI version of this header (bumped on any signature change). */
int fqtk_abi_version(void);

/* Number of visible HIP devices (0 without a GPU; FQTK_OK either way). */
int fqtk_device_count(int *n_devices);

/* Replaces `BarcodeMatcher::new(samples, max_mismatches, min_mismatch_delta, use_cache)`
 * (barcode_matching.rs:55-86; sole call site demux.rs:921-926).  `barcodes[s]` are NUL-terminated
 * ASCII strings of exactly `barcode_len` bytes; they are upper-cased and encoded like the reference
 * does (:71-75) and copied -- the caller keeps ownership.  `use_cache` has its own setter below
 * (default on, like demux.rs:925); the complete memo table is built here, on the device.  Errors: n_samples == 0 ("Must provide at least one
 * sample"), empty barcode ("Sample barcode cannot be empty string"), unequal lengths (the reference
 * would panic on the first assign), barcode_len > FQTK_MAX_BARCODE_LEN, n_samples >
 * FQTK_MAX_SAMPLES -> FQTK_EINVAL; no device -> FQTK_ENODEV. */
int fqtk_matcher_create(const char *const *barcodes, uint32_t n_samples, uint32_t barcode_len,
                        uint8_t max_mismatches, uint8_t min_mismatch_delta, int device,
                        fqtk_matcher **out);

void fqtk_matcher_destroy(fqtk_matcher *m);

/* Optional: the `sample_id` of each sample (Sample.sample_id, samples.rs:19), in table order; copied.
 * Only used to word FQTK_ELEN messages exactly like the reference's panic, which names the sample
 * (barcode_matching.rs:95-107).  Without it samples are called "sample_<index>", as the reference's own
 * test helper names them (barcode_matching.rs:195-211).  NULL clears. */
int fqtk_matcher_set_sample_ids(fqtk_matcher *m, const char *const *sample_ids);

/* Introspection (fields of BarcodeMatcher, barcode_matching.rs:29-45). */
uint32_t fqtk_matcher_n_samples(const fqtk_matcher *m);
uint32_t fqtk_matcher_barcode_len(const fqtk_matcher *m);
uint32_t fqtk_matcher_max_ns_in_barcodes(const fqtk_matcher *m); /* :73-74 */
int fqtk_matcher_device(const fqtk_matcher *m);

/* Replaces the `use_cache` argument/field of BarcodeMatcher (barcode_matching.rs:41-42,59; demux
 * passes true, demux.rs:925).  The reference's cache is a lazily filled AHashMap of Some results
 * keyed on the read bytes (:174-181); here it is a COMPLETE table, precomputed at create time on the
 * device, of every canonical (A/C/G/T/N) read within max_mismatches of a sample -- so a miss proves
 * None.  Default 1.  0 forces the exhaustive per-sample scan for every read.  Results are identical
 * either way (as in the reference).  The table is absent (scan only) when barcode_len > 20 or the
 * candidate set exceeds the build budget; fqtk_matcher_memo_entries() then returns 0. */
int fqtk_matcher_set_use_cache(fqtk_matcher *m, int use_cache);
uint64_t fqtk_matcher_memo_entries(const fqtk_matcher *m);
uint64_t fqtk_matcher_memo_candidates(const fqtk_matcher *m);

/* Where the memo lives (tuning / test knob, no counterpart in the reference; results never depend on it).
 *   FQTK_MEMO_NONE   no memo: every read takes the exhaustive scan
 *   FQTK_MEMO_TABLE  two-choice hash table in HBM/L2 + LDS hot subset (any sample alphabet, any max_mismatches)
 *   FQTK_MEMO_LDS    one-dword entries, whole table resident in each CU's LDS -- built when all sample
 *                    barcodes are plain A/C/G/T, max_mismatches <= 1 and the table fits 160 KiB; for barcodes
 *                    of 17-32 bases whose dwords do not fit (384 samples x 12+12), three-byte entries behind a
 *                    minimal perfect hash
 * fqtk_matcher_memo_kind() reports the form the next batch will use; fqtk_matcher_set_memo_kind(m,
 * FQTK_MEMO_TABLE) pins the HBM/L2 form, FQTK_MEMO_LDS (the default) means "best available". */
#define FQTK_MEMO_NONE 0
#define FQTK_MEMO_TABLE 1
#define FQTK_MEMO_LDS 2
int fqtk_matcher_memo_kind(const fqtk_matcher *m);
int fqtk_matcher_set_memo_kind(fqtk_matcher *m, int kind);
/* FQTK_MEMO_TABLE has a direct-indexed variant for barcodes of <= 10 bases: reads without a no-call index a
 * flat result array by their own 2-bit base codes (no hash, no probe sequence), an LDS cache holds its
 * exact-match entries, and only reads with an N go to the hash table.  Returns the bytes per array entry
 * (2 or 4) when that variant is what FQTK_MEMO_TABLE means for this matcher, else 0. */
int fqtk_matcher_memo_direct_bytes(const fqtk_matcher *m);

/* Which kernel runs the exhaustive scan (tuning / test knob, no counterpart in the reference; results never depend on it).
 * The scan serves every read when there is no memo (FQTK_MEMO_NONE: use_cache 0, barcode_len > 20 without an LDS form, a
 * candidate set over the build budget -- e.g. max_mismatches 3 on 384 x 16).
 *   FQTK_SCAN_VALU  one lane per read, the table in SGPRs: 8 VALU instructions per (read, sample, 32 bases)
 *   FQTK_SCAN_MFMA  int8 matrix instructions count the mismatches of 32 reads x 32 samples at a time and make the packed
 *                   (mismatches, index) key in the accumulator; any barcode_len, at most 16384 samples
 * fqtk_matcher_scan_kind() reports what the next scanned batch runs; fqtk_matcher_set_scan_kind(m, FQTK_SCAN_MFMA) pins
 * the matrix form (FQTK_EINVAL when the table has more than 16384 samples), FQTK_SCAN_VALU the other.  The environment
 * variable FQTK_SCAN (valu / mfma), read by fqtk_matcher_create, sets the same; unset, the matcher chooses. */
#define FQTK_SCAN_VALU 0
#define FQTK_SCAN_MFMA 1
int fqtk_matcher_scan_kind(const fqtk_matcher *m);
int fqtk_matcher_set_scan_kind(fqtk_matcher *m, int kind);

/* Replaces one `BarcodeMatcher::assign(&mut self, read_bases: &[u8]) -> Option<BarcodeMatch>` call
 * per template (barcode_matching.rs:165-186; sole call site demux.rs:968) with one call per batch.
 * HOST pointers; synchronous.
 *   obs      n x stride ASCII bytes, read i at obs + i*stride (the SoA form of
 *            ReadSet::sample_barcode_sequence, demux.rs:121-123)
 *   obs_len  per-read length, or NULL when every read has exactly barcode_len bases
 *            (stride must then be >= barcode_len); obs_len[i] <= stride is CHECKED here (FQTK_EINVAL).
 *            With obs_len the memo still serves every read of length barcode_len; shorter reads are
 *            None, longer ones None or FQTK_ELEN (rules above).  stride < barcode_len is legal with
 *            obs_len: every read is then shorter than a barcode and every result None.
 *   out      n results
 *   counts   NULL, or S+1 counters that are ADDED to: counts[idx] for Some, counts[S] for None --
 *            the per-sample `templates` metric of demux.rs:970-974
 * Returns FQTK_ELEN when some read is longer than barcode_len and not rejected by the no-call
 * prefilter; results for the other reads are still written.  fqtk_last_error() is then the
 * reference's panic sentence for the lowest such read (barcode_matching.rs:95-107),
 *   "Read barcode (<decoded read>) length (<n>) differs from expected barcode (<sample 0's barcode>)
 *    length (<L>) for sample <sample 0's id>"   followed by " [read index <i> of its batch]".
 * Uses two pipeline slots of its own: chunks a caller has in flight on slots 0..FQTK_MAX_SLOTS-1 are
 * neither waited on nor disturbed. */
int fqtk_matcher_assign_batch(fqtk_matcher *m, const uint8_t *obs, uint32_t stride,
                              const uint32_t *obs_len, uint64_t n, fqtk_match_t *out,
                              uint64_t *counts);

/* Same, but every pointer is a DEVICE pointer on the matcher's device and the work is enqueued on
 * `hip_stream` (a hipStream_t, NULL = the default stream) without synchronising: the zero-copy form
 * used when reads are already resident in HBM.  d_counts: NULL or S+1 uint64 accumulated with
 * atomics.  Length errors are latched in the handle; collect them with fqtk_matcher_poll_error().
 * d_obs_len[i] <= stride is the caller's contract here (device memory is not inspected on the host);
 * the kernels clamp every access to the read's row regardless.
 * Device memory the handle may add behind this call: once a read with an IUPAC / junk byte has been met, a
 * worklist of up to n bytes per stream in use (n / 4 read indices; grown on demand, freed with the handle). */
int fqtk_matcher_assign_batch_device(fqtk_matcher *m, const void *d_obs, uint32_t stride,
                                     const void *d_obs_len, uint64_t n, void *d_out, void *d_counts,
                                     void *hip_stream);

/* Synchronises `hip_stream`, then reports and clears the latched length error of earlier
 * *_device / enqueue calls: FQTK_OK, or FQTK_ELEN with the lowest offending read index of the
 * batch that raised it in *read_index (may be NULL). */
int fqtk_matcher_poll_error(fqtk_matcher *m, void *hip_stream, uint64_t *read_index);

/* Scalar convenience with the reference's exact call shape (one read in, Option out): returns
 * FQTK_OK and writes *out (idx == FQTK_NO_MATCH for None), or FQTK_ELEN. */
int fqtk_matcher_assign1(fqtk_matcher *m, const uint8_t *read_bases, uint32_t len,
                         fqtk_match_t *out);

/* ---- pinned-buffer pipeline: decompress -> match -> write overlap (north_star) --------------- */
/* Page-locked host memory for the SoA chunk buffers so H2D/D2H run as async DMA. */
int fqtk_pinned_alloc(size_t bytes, void **out);
int fqtk_pinned_free(void *p);

#define FQTK_MAX_SLOTS 8
/* Enqueue one chunk on pipeline slot `slot` (0..FQTK_MAX_SLOTS-1; each slot = its own HIP stream +
 * device staging): async H2D of obs (and obs_len if non-NULL), kernel, async D2H into `out`.
 * Returns immediately.  Buffers must stay valid (and should be pinned) until fqtk_matcher_wait().
 * Per-sample counts are accumulated on the device; read them with fqtk_matcher_counts(). */
int fqtk_matcher_enqueue(fqtk_matcher *m, int slot, const uint8_t *obs, uint32_t stride,
                         const uint32_t *obs_len, uint64_t n, fqtk_match_t *out);
/* ---- packed input: 4 bits per base over PCIe instead of 8 ------------------------------------------------------
 * A packed row holds base k of the barcode in nibble k (byte k / 2, low nibble first); codes A 0, C 1, T 2, G 3 and 7
 * for the no-calls N, n and '.' (mod.rs:85-87) -- lower case like upper case, as the reference's encode() treats it
 * (mod.rs:49-61).  Rows are fqtk_packed_stride(barcode_len) bytes apart (the nibbles rounded up to 4 bytes: 8 + 8
 * bases -> 8 bytes).  A read with any other byte (an IUPAC code, junk) cannot be carried in 4 bits: the packer lists it
 * as an EXCEPTION -- its index and its barcode_len ASCII bytes -- and the enqueue call puts those rows back in place on
 * the device, so results are those of the ASCII entry points for every input.
 *
 * fqtk_pack_barcodes: host-side packer (plain CPU code: one table look-up per base; run it in the threads that produce
 * the barcodes).  obs: n x stride ASCII rows as for fqtk_matcher_enqueue; exc_index / exc_rows: room for exc_cap
 * exceptions (exc_cap * barcode_len bytes of rows), *n_exc = how many there are; FQTK_ENOMEM if they do not fit. */
uint32_t fqtk_packed_stride(uint32_t barcode_len);
int fqtk_pack_barcodes(const uint8_t *obs, uint32_t stride, uint32_t barcode_len, uint64_t n, uint8_t *packed,
                       uint32_t packed_stride, uint32_t *exc_index, uint8_t *exc_rows, uint64_t exc_cap, uint64_t *n_exc);
/* fqtk_matcher_enqueue for packed rows (every read exactly barcode_len bases: no obs_len form): async H2D of the packed
 * rows and the exceptions, unpack to ASCII rows in HBM, the same kernels as every other entry point, async D2H into
 * `out`; fqtk_matcher_wait(slot) completes it, counts accumulate as for fqtk_matcher_enqueue.  Replaces one `assign`
 * per template (demux.rs:968) like fqtk_matcher_enqueue does, at 8 + 4 instead of 16 + 4 bytes per read over the link
 * for 8 + 8-base dual indexes. */
int fqtk_matcher_enqueue_packed(fqtk_matcher *m, int slot, const uint8_t *packed, uint32_t packed_stride, uint64_t n,
                                const uint32_t *exc_index, const uint8_t *exc_rows, uint64_t n_exc, fqtk_match_t *out);

/* Blocks until the chunk on `slot` is complete; FQTK_ELEN as for assign_batch.  Every slot latches its
 * own error: the status belongs to the chunk that was enqueued on THIS slot. */
int fqtk_matcher_wait(fqtk_matcher *m, int slot);
/* Adds the device-side accumulated counts (S+1) of all completed enqueue() chunks into `counts`
 * and resets the device accumulator.  Synchronises all slots. */
int fqtk_matcher_counts(fqtk_matcher *m, uint64_t *counts);

/* ---- census of the unmatched barcodes: which barcodes did the None reads carry? ----------------------------------
 * No counterpart in the reference (its only figure is the `unmatched` row of demux-metrics.txt, counts[S] here).  Opt-in,
 * owned by the handle: a device-resident table of (barcode, count) over every read whose result is None, accumulated over
 * every batch of every entry point above (and of the record pipeline of fqtk_demux.h, which runs its batches through
 * fqtk_matcher_assign_batch_device) by one more kernel behind the batch's own, on the batch's stream.  OFF (the default):
 * no kernel is launched, no memory is taken and every result, count and error is what it is without these entry points.
 *   keyed    a None read of exactly barcode_len bases (no obs_len, or obs_len[i] == barcode_len) none of whose first
 *            barcode_len bytes enc() maps to 0.  Its KEY is its enc() string, 4 bits a base: lower case is upper case, 'N' 'n'
 *            '.' are N, U is T, IUPAC codes keep their mask; two reads are the same barcode iff their keys are equal, and the
 *            barcode is reported as the reference's decode() spells the key (mod.rs:68): barcode_len letters of
 *            ACGTMRWSYKVHDBN.  Reads the no-call prefilter rejects are keyed like any other; all-N is an ordinary entry.
 *   unkeyed  every other None read -- shorter or longer than barcode_len (a read that raises FQTK_ELEN too), one with a junk
 *            byte, every read of a batch with stride < barcode_len -- adds 1 to one counter.
 *   overflow the table has `capacity` slots, fixed at enable.  A read whose key finds no slot within the kernel's bounded
 *            probe sequence adds 1 to `overflow` and is not stored.
 * A barcode that is reported carries its EXACT count and is reported once: slots only ever go from empty to a key, probing
 * is deterministic, so a key that was dropped once is dropped every time.  At any quiescent point
 *   keyed + unkeyed + overflow == number of None results produced since enable / reset,   keyed = sum of the stored counts.
 * barcode_len <= 32 (one or two 64-bit key words; covers 8 + 8 .. 16 + 16 dual indexes).
 * Device memory (what rocm-smi shows for the process grows by this at enable): capacity x 16 bytes for barcode_len <= 16,
 * capacity x 24 above; the default of 2^20 slots is 16 / 24 MiB.  A read-out adds, while it runs, 24 bytes per distinct barcode.
 *
 * enable: capacity_slots is rounded up to a power of two, 0 = 2^20; allocates and clears (again with another capacity:
 * re-allocates and clears).  FQTK_EINVAL when barcode_len > 32 or capacity_slots > 2^32; FQTK_ENOMEM.
 * disable frees the table (fqtk_matcher_destroy does, too); reset clears the table and the totals.  All three wait for the
 * device to drain first. */
int fqtk_matcher_census_enable(fqtk_matcher *m, uint64_t capacity_slots);
int fqtk_matcher_census_disable(fqtk_matcher *m);
int fqtk_matcher_census_reset(fqtk_matcher *m);
/* The two read-outs synchronise the device first, leave the census as it is, and return FQTK_EINVAL ("census is not enabled")
 * when it is off.  totals: distinct = barcodes stored; any pointer may be NULL. */
int fqtk_matcher_census_totals(fqtk_matcher *m, uint64_t *distinct, uint64_t *keyed, uint64_t *unkeyed, uint64_t *overflow);
/* top: the k most frequent barcodes, count descending, ties by the barcode ascending (bytewise).  barcodes: room for
 * k x barcode_len bytes, row i at barcodes + i * barcode_len, no NUL; counts: k; *n_out = rows written = min(k, distinct).
 * Only the `distinct` entries cross the link; the order is made on the host. */
int fqtk_matcher_census_top(fqtk_matcher *m, uint32_t k, char *barcodes, uint64_t *counts, uint32_t *n_out);

/* ---- index pairs of the unmatched reads: which index-1 x index-2 combinations did the None reads carry? ------------
 * The index-hopping / swapped-plate / wrong-sample-sheet report of a dual-index run; no counterpart in the reference.
 * Opt-in, owned by the handle, accumulated over every batch of every entry point like the census above, by one more kernel
 * behind the batch's own on the batch's stream.  OFF (the default): no kernel is launched, no memory is taken and every
 * result, count and error is what it is without these entry points.  With the census on as well, both run.
 *   A, B     the distinct strings barcode_s[0 : len_a] and barcode_s[len_a : barcode_len] of the table (upper case, as the
 *            matcher keeps it), each in order of first appearance; U_A and U_B of them.
 *   assign   each index of a read is assigned on its own with the matcher's rule applied to that index's positions and that
 *            list: mismatches counted as enc(read) & ~enc(index) != 0, best = the lowest count, idx = the lowest entry that has
 *            it, next = the second smallest with multiplicity (255 for a list of one); unassigned when
 *            best > max_mismatches or next - best < min_mismatch_delta (the two parameters given here, per index).
 *            No special cases: N, lower case, '.', IUPAC codes and bytes that encode to 0 count as they do in the whole rule.
 *   tallied  every None read of exactly barcode_len bases (stride >= barcode_len, and no obs_len or obs_len[i] ==
 *            barcode_len) adds 1 to cell [a][b] of a (U_A + 1) x (U_B + 1) matrix of 64-bit counters; row U_A and column
 *            U_B mean "this index unassigned".  A cell whose pair is a sample's own barcode is legal (one error in each index
 *            with max_mismatches 1, say) and is reported.
 *   skipped  every other None read adds 1 to one counter.
 * At any quiescent point   sum(matrix) + skipped == number of None results produced since enable / reset.
 * Device memory: 8 bytes a cell and 16 bytes per distinct index.
 *
 * enable: builds A, B and their planes, allocates and clears the matrix (again: with the new parameters, cleared).
 * FQTK_EINVAL when barcode_len > 32, when len_a == 0 or len_a >= barcode_len, or when the matrix would have more than 2^24
 * cells (128 MiB); FQTK_ENOMEM.  disable frees everything (fqtk_matcher_destroy does, too); reset clears the matrix and
 * `skipped`.  All three wait for the device to drain first. */
int fqtk_matcher_pairs_enable(fqtk_matcher *m, uint32_t len_a, uint32_t max_mismatches, uint32_t min_mismatch_delta);
int fqtk_matcher_pairs_disable(fqtk_matcher *m);
int fqtk_matcher_pairs_reset(fqtk_matcher *m);
/* The read-outs return FQTK_EINVAL ("the index-pair tally is not enabled") when it is off.  dims: U_A and U_B.  index: entry i
 * of A (which = 0) or B (which = 1) as a NUL-terminated string; out has room for barcode_len bytes.  read: synchronises the
 * device and copies the matrix, row-major with (U_A + 1) * (U_B + 1) cells, and `skipped`; either pointer may be NULL; the
 * tally stays as it is. */
int fqtk_matcher_pairs_dims(fqtk_matcher *m, uint32_t *u_a, uint32_t *u_b);
int fqtk_matcher_pairs_index(fqtk_matcher *m, int which, uint32_t i, char *out);
int fqtk_matcher_pairs_read(fqtk_matcher *m, uint64_t *matrix, uint64_t *skipped);

/* ---- indel rescue of the unmatched reads: one inserted or deleted base shifts every base behind it ------------------
 * Every rule above counts substitutions only, so a read with an indel inside its index sits many mismatches from its own
 * sample and comes out None.  No counterpart in the reference.  Opt-in, owned by the handle: one more kernel behind a batch's
 * own, on the batch's stream and IN FRONT of the census and the pair tally, gives the None reads of exactly barcode_len bases
 * (stride >= barcode_len, and no obs_len or obs_len[i] == barcode_len) a second look under an edit-distance rule; out[], the
 * counts, the census, the pair tally and the record pipeline of fqtk_demux.h see the rescued result.  OFF (the default): no
 * kernel is launched, no memory is taken, every result is what it is without these entry points.  The weighted calls below are
 * never rescued.  The rule, all integer, L = barcode_len:
 *   mis(r, s) = enc(r) & ~enc(s) != 0     (enc as everywhere else; a byte that encodes to 0 never mismatches)
 *   D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + mis(read[i-1], sample[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
 *   dist = min(min over j of D[L][j], min over i of D[i][L])      the sequence-Levenshtein distance: the last row takes an
 *          inserted base (the barcode's tail is pushed out of the read), the last column a deleted one (adapter bases pulled in)
 *   sat = max_edits + max(min_edit_delta, 1); every distance is taken as min(dist, sat), which changes no decision (with a
 *          delta of 0 the cap sits one above max_edits, so that a capped distance is never accepted)
 *   best = the lowest distance, idx = the LOWEST s that has it, next = the second smallest with multiplicity (sat for a table
 *   of one sample); the read STAYS None iff best > max_edits or next - best < min_edit_delta, and is then not written at all.
 * A rescued read: idx = s, best = 0x80 | best, next = next -- bit 7 of `best` says "an edit distance, not a mismatch count"
 * (so the read is neither a perfect nor a one-mismatch match to whoever reads `best`).  With counts: +1 at s, -1 at S.
 * The handle's own counters: rescued[s] = reads rescued into s, rescued[S] = reads examined and left None; skipped = None reads
 * of another length.  Per batch with stride >= barcode_len:  sum(rescued) + skipped == None results of the matcher's kernels.
 * Device memory: 64 bytes per sample and four bases, 8 bytes per sample.
 *
 * enable: FQTK_EINVAL when barcode_len > 32, when max_edits + min_edit_delta is 0 or above 16, or when max_edits >=
 * barcode_len (the matcher stays as it was); FQTK_ENOMEM.  Again: the new parameters, counters cleared.  disable frees
 * everything (fqtk_matcher_destroy does, too); reset clears the counters.  All three wait for the device to drain first.
 * read: synchronises the device and copies rescued (S + 1) and skipped; either pointer may be NULL.  After disable it returns
 * the counters as disable found them, until the next enable; FQTK_EINVAL ("the indel rescue is not enabled") before any enable. */
int fqtk_matcher_indel_enable(fqtk_matcher *m, uint32_t max_edits, uint32_t min_edit_delta);
int fqtk_matcher_indel_disable(fqtk_matcher *m);
int fqtk_matcher_indel_reset(fqtk_matcher *m);
int fqtk_matcher_indel_read(fqtk_matcher *m, uint64_t *rescued, uint64_t *skipped);

/* ---- quality-weighted assignment: a mismatch costs what the sequencer said about that base ---------------------------
 * No counterpart in the reference, whose rule counts every mismatch as 1.  Here (all integer):
 *   w[i]    = clamp(qual[i] - 33, 0, 93)        every byte value is defined: below '!' is 0, above '~' is 93
 *   cost[s] = sum over i < barcode_len of  w[i] * [ enc(read[i]) & ~enc(barcode_s[i]) != 0 ]      (enc as everywhere else)
 *   best = the lowest cost, idx = the LOWEST s that has it, next = the second smallest with multiplicity (0xFFFF for a
 *   table of one sample);   None  iff  best > max_cost  or  next - best < min_cost_delta.
 * A read byte that enc() maps to 0 never mismatches; a no-call costs its own quality against every sample base that is not N.
 * With every quality equal to q, cost = q * mismatches: max_cost = q * mm + q - 1 and min_cost_delta = q * delta make the
 * decisions of max_mismatches = mm, min_mismatch_delta = delta.
 * The answer depends on the qualities, so no memo serves it: every read takes the scan of weighted_scan_kernels.hip.h (int8
 * matrix cores).  Scope: every read has exactly barcode_len bases (no obs_len form), barcode_len <= 32 (a cost is at most
 * 32 * 93 = 2976), n_samples <= 16384.  The matcher's max_mismatches / min_mismatch_delta play no part in these calls, and
 * these calls none in the others: set_weighted changes nothing for any other entry point.
 *
 * set_weighted: sets (or changes) the two bounds and turns the two calls below on.  FQTK_EINVAL for barcode_len > 32 or
 * n_samples > 16384.
 * assign_weighted_batch: host pointers, synchronous, on a pipeline slot of its own like fqtk_matcher_assign_batch.  obs and
 * qual are n rows `stride` bytes apart each (stride >= barcode_len; what follows the barcode in a row is not looked at).
 *   out[i]    idx, best = min(best cost, 255), next = min(next cost, 255); idx == FQTK_NO_MATCH (all bits set) for None
 *   costs     NULL, or n words: best cost | next cost << 16, 0xFFFFFFFF for None
 *   counts    NULL, or S+1 counters that are ADDED to, as for fqtk_matcher_assign_batch
 * assign_weighted_batch_device: the same with DEVICE pointers, enqueued on `hip_stream` without synchronising; d_counts NULL
 * or S+1 uint64 accumulated with atomics.  Nothing is latched: there is no length error to raise.
 * FQTK_EINVAL: before set_weighted, qual (or obs, out) NULL, stride < barcode_len.
 * With the census or the index-pair tally enabled they run behind a weighted batch as behind any other and see its None
 * results; the pair tally keeps its own UNWEIGHTED per-index rule (fqtk_matcher_pairs_enable's two parameters). */
int fqtk_matcher_set_weighted(fqtk_matcher *m, uint32_t max_cost, uint32_t min_cost_delta);
int fqtk_matcher_assign_weighted_batch(fqtk_matcher *m, const uint8_t *obs, const uint8_t *qual, uint32_t stride, uint64_t n,
                                       fqtk_match_t *out, uint32_t *costs, uint64_t *counts);
int fqtk_matcher_assign_weighted_batch_device(fqtk_matcher *m, const void *d_obs, const void *d_qual, uint32_t stride, uint64_t n,
                                              void *d_out, void *d_costs, void *d_counts, void *hip_stream);

/* ---- per-index mismatch budgets: each index of a dual-index read is matched on its own -----------------------------------
 * Every rule above counts mismatches over the whole concatenated barcode.  This is the other rule, the one bcl2fastq and BCL
 * Convert apply (--barcode-mismatches 1,1): no counterpart in the reference.  All integer; L = barcode_len.
 *   parameters  len_a with 0 < len_a < L; (mm_a, delta_a) for index 1 = positions [0, len_a); (mm_b, delta_b) for index 2 = [len_a, L)
 *   A, B        the distinct strings barcode_s[0 : len_a] and barcode_s[len_a : L], each in order of first appearance: exactly
 *               the lists of fqtk_matcher_pairs_enable above
 *   per index   assigned against its list by the text under "assign" in the pairs section: a mismatch is
 *               enc(read) & ~enc(index) != 0, best = the lowest count, the entry = the lowest one that has it, next = the second
 *               smallest with multiplicity (255 for a list of one); the index is unassigned when best > mm_i or
 *               next - best < delta_i.  No special cases for any byte value.
 *   the read    None when either index is unassigned or when no sample has the pair (a, b); else idx = the LOWEST s with that
 *               pair, best = best_a + best_b, next = min(255, min(next_a + best_b, best_a + next_b)).
 * Scope: every row holds exactly L bases (stride >= L, no obs_len form), L <= 32, len_a <= 16 and L - len_a <= 16.  The matcher's
 * max_mismatches / min_mismatch_delta play no part in these calls, and these calls none in the others.
 * How it runs (results never depend on it): for plain A/C/G/T tables with mm_a, mm_b <= 1 whose image fits, two per-index memos,
 * the index keys and a pair -> sample directory are resident in every CU's LDS and a read is two LDS look-ups
 * (FQTK_PER_INDEX_LDS); every other table takes a per-index scan of each read (FQTK_PER_INDEX_SCAN).
 * fqtk_matcher_per_index_kind() reports what the next batch runs (FQTK_PER_INDEX_OFF before set_per_index);
 * fqtk_matcher_set_per_index_kind(m, FQTK_PER_INDEX_SCAN) pins the scan, FQTK_PER_INDEX_LDS means "best available": a tuning / test
 * knob like fqtk_matcher_set_memo_kind, of no use to a caller who only wants results.
 *
 * set_per_index: builds A, B, the scan tables and the LDS image (again: with the new parameters).  FQTK_EINVAL for L > 32,
 * len_a == 0 or >= L, an index longer than 16 bases (the matcher stays as it was); FQTK_ENOMEM.  Before it nothing is allocated
 * and nothing is launched.  Device memory: 16 bytes per distinct index, 4 per distinct pair, at most 160 KiB of image.
 * assign_per_index_batch: host pointers, synchronous, on a pipeline slot of its own like fqtk_matcher_assign_batch; counts NULL
 * or S+1 counters that are ADDED to.  assign_per_index_batch_device: DEVICE pointers, enqueued on `hip_stream` without
 * synchronising; d_counts NULL or S+1 uint64 accumulated with atomics.  Nothing is latched: there is no length error to raise.
 * FQTK_EINVAL: before set_per_index, obs / out NULL, stride < barcode_len.
 * With the census or the index-pair tally enabled they run behind such a batch as behind any other and see its None results
 * (the pair tally keeps the two parameters of fqtk_matcher_pairs_enable).  The indel rescue never touches these calls. */
#define FQTK_PER_INDEX_OFF 0
#define FQTK_PER_INDEX_SCAN 1
#define FQTK_PER_INDEX_LDS 2
int fqtk_matcher_set_per_index(fqtk_matcher *m, uint32_t len_a, uint32_t mm_a, uint32_t delta_a, uint32_t mm_b, uint32_t delta_b);
int fqtk_matcher_per_index_kind(const fqtk_matcher *m);
int fqtk_matcher_set_per_index_kind(fqtk_matcher *m, int kind);
int fqtk_matcher_assign_per_index_batch(fqtk_matcher *m, const uint8_t *obs, uint32_t stride, uint64_t n, fqtk_match_t *out, uint64_t *counts);
int fqtk_matcher_assign_per_index_batch_device(fqtk_matcher *m, const void *d_obs, uint32_t stride, uint64_t n, void *d_out, void *d_counts,
                                               void *hip_stream);

/* ---- several GPUs in one process------------------------------------------------ */
/* Templates are independent, so chunks shard over devices with no data-path exchange: one matcher per
 * device (the table is replicated by fqtk_matcher_create), chunk k goes to matcher k mod n.  The ONE
 * collective of the path is the end-of-run reduction of the per-sample counts (the `templates` column of
 * demux-metrics.txt, demux.rs:970-974, 994-998): this call all-reduces the enqueue()/wait() accumulators of
 * `n` matchers living on `n` DISTINCT devices with RCCL (ncclAllReduce, ncclUint64, ncclSum over xGMI; the
 * library is loaded with dlopen on first use), ADDS the total into counts[0..S] and resets every
 * accumulator -- what fqtk_matcher_counts does for one matcher.  With n == 1 no collective is needed and
 * none is made unless `force_collective` is non-zero (a one-rank communicator; exercises the RCCL path
 * on a single-GPU box).  All matchers must have the same number of samples. */
int fqtk_matchers_allreduce_counts(fqtk_matcher *const *matchers, int n, int force_collective, uint64_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* FQTK_MATCH_H */
