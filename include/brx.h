/*
 * brx.h -- C ABI of the MI355X-native replacement for natir/br's hot path:
 * solid-k-mer set build (count -> threshold -> packed canonical bitset) and the
 * per-read correction scan (br::correct::{One,Two,Graph,Greedy,GapSize} against
 * br::set::KmerSet).
 *
 * The reference (Rust, /root/reference) has no FFI layer; its seam is two traits
 * and two free functions.  Each entry point below names the reference interface it
 * replaces (file:line under /root/reference).  INTEGRATION.md shows the Rust-side
 * binding (`impl KmerSet for HipSet`, `run_correction` calling the batch entry).
 *
 * Conventions
 *   - every function returns 0 (BRX_OK) or a negative brx_status; nothing unwinds;
 *     brx_last_error() gives a thread-local message for the last failure.
 *   - "bases/offsets" batches: reads concatenated as ASCII bytes, read r =
 *     bases[offsets[r] .. offsets[r+1]); offsets has n_reads+1 entries.
 *   - k-mers are FORWARD 2-bit k-mers (A=0 C=1 T=2 G=3, first base most
 *     significant, 2k low bits) exactly as `KmerSet::get` receives them; the
 *     library canonicalises (even-popcount member of {kmer, revcomp}) and indexes
 *     bit (canonical >> 1), like pcon::solid::Solid.
 *   - `_device` variants take device pointers (HIP, same device as the handle) and a
 *     hipStream_t passed as void*; the plain variants take host pointers and do the
 *     transfers themselves.
 *   - a brx_set_t is immutable once built/loaded and may be shared by any number of
 *     chains; a brx_chain_t owns its workspace and serialises concurrent calls.
 *   - what a set IS is the reference's: the canonical k-mers with `KmerSet::get` = true.
 *     How it is HELD in HBM varies (bit vector for k <= 19, possibly lazy; key list +
 *     probe index; sparse table for k >= 21) and never changes an answer -- see
 *     brx_set_bits_state / brx_set_sparse / brx_set_index_* below and DESIGN.md 3, 5.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry
 *     returns BRX_ERR_NODEVICE.
 */
#ifndef BRX_H
#define BRX_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct brx_set brx_set_t;         /* Box<dyn KmerSet> backed by set::Pcon   src/set.rs:17-23, src/set/pcon.rs:13-15 */
typedef struct brx_counter brx_counter_t; /* pcon::counter::Counter<u8>             src/main.rs:73-78 */
typedef struct brx_chain brx_chain_t;     /* Vec<Box<dyn Corrector>> of build_methods  src/lib.rs:141-164 */

typedef enum brx_status {
    BRX_OK = 0,
    BRX_ERR_ARG = -1,         /* bad argument (k even/out of range, null pointer, ...) */
    BRX_ERR_NOMEM = -2,       /* host or device allocation failed                      */
    BRX_ERR_HIP = -3,         /* a HIP runtime call failed                             */
    BRX_ERR_NODEVICE = -4,    /* no usable GPU: the product path has no CPU fallback   */
    BRX_ERR_FORMAT = -5,      /* malformed .solid stream or key file (error.rs: wraps pcon errors) */
    BRX_ERR_UNSUPPORTED = -6, /* valid in the reference, not yet implemented here      */
    BRX_ERR_OVERFLOW = -7     /* caller-provided output buffer too small               */
} brx_status;

/* CorrectionMethod, src/cli.rs:11-17; order = build_methods' match, src/lib.rs:150-160 */
enum { BRX_ONE = 0, BRX_TWO = 1, BRX_GRAPH = 2, BRX_GREEDY = 3, BRX_GAP_SIZE = 4 };

/* one entry of the method list handed to build_methods (src/lib.rs:141-146):
 * confirm = -C (default 5, src/cli.rs:135-137), max_search = -M (default 7, :140-142) */
typedef struct brx_method {
    uint8_t method;
    uint8_t confirm;
    uint8_t max_search;
} brx_method_t;

/* ---- diagnostics -------------------------------------------------------------------- */
const char *brx_strerror(int status);
const char *brx_last_error(void);
int brx_version(void);
int brx_device_count(int *n); /* BRX_OK and *n == 0 when no GPU is visible */

/* per-kernel HIP-event timers (events recorded on the launch stream).  Names:
 * "count_dense", "threshold", "correct_pass", "compact", "cover", ... */
int brx_profile_enable(int on);
int brx_profile_reset(void);
int brx_profile_get(const char *kernel, double *total_ms, uint64_t *launches);
int brx_profile_names(char *buf, size_t cap); /* comma-separated list of timer names */

/* ---- KmerSet: src/set.rs:17-21 --------------------------------------------------------- */
/* Pcon::new(Solid::new(k)): empty set                              src/set/pcon.rs:183-185 */
int brx_set_new(uint8_t k, int device, brx_set_t **out);
/* Pcon::from_pcon_solid: [k:u8][bits Lsb0], already decompressed   src/set/pcon.rs:18-25   */
int brx_set_new_from_solid_bytes(const uint8_t *buf, size_t len, int device, brx_set_t **out);
/* Pcon::from_fasta (presence only): OR in every canonical k-mer of every read of length >= k
 *                                                                  src/set/pcon.rs:47-112  */
int brx_set_insert_batch(brx_set_t *set, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads);
/* ---- streams: what every entry with a `void *stream` argument promises (tests/test_gpu_streams.py holds it to this) ----
 * `stream` is a hipStream_t of the handle's device; NULL is the legacy null stream, like any HIP API.  The caller's streams
 * may be non-blocking (hipStreamNonBlocking: no implicit ordering with the null stream), as the library's own are.
 *   - INPUTS need only be ready in the order of `stream`: device buffers may still be being written by work queued on
 *     `stream` before the call.  The library reads them, and everything it derives from them, on `stream`.
 *   - RESULTS are ready in the order of `stream` -- work queued on `stream` after the call sees them; the host sees them
 *     after it has synchronised `stream` -- or on return, where the entry says that it returns after its kernels have
 *     completed or after `stream` has been synchronised.  Values handed back through host pointers are valid on return.
 *   - a FRESHLY CREATED object (brx_set_new, brx_set_count_begin, brx_set_count_finish, brx_set_load_fd, brx_set_combine, brx_chain_new) may
 *     be used on any stream at once: whatever its constructor zeroes or writes is complete when the constructor returns.
 *   - an entry WITHOUT a stream argument that changes an object (brx_set_count_add_batch, brx_counter_load_counts,
 *     brx_counter_load_fd, brx_count_fasta_fd) sees everything that earlier calls on the same object enqueued, whichever stream they named:
 *     brx_counter_reset(c, s) followed by brx_set_count_add_batch(c, ..) counts into the emptied counter although the batch
 *     runs on the counter's own stream, and brx_set_count_finish_into(c, a, s, dst); brx_counter_reset(c, s) followed by it
 *     leaves the finish queued on `s` its batches and workspace, for every count strategy.  The same holds for the counter's
 *     host-path lookups (brx_counter_abundance_batch, brx_counter_get_counts, brx_counter_save_fd).
 *   - the host-path READERS of a set -- brx_set_get, get_batch, get_batch_indexed, popcount, export_solid_bytes, set,
 *     brx_set_save_fd, brx_set_combine, brx_set_compare -- work on the null stream or one of their own and do NOT wait for a non-blocking stream: after an asynchronous device
 *     entry that wrote the set (insert_batch_device, or_keys_device, count_finish_into) the ordering is the CALLER's:
 *     synchronise that stream first.  Pointers handed out (brx_set_device_bits, brx_set_keylist_device,
 *     brx_counter_device_counts, brx_counter_l1_view) are the caller's to order likewise.
 *   - state that is built on first use (a lazy bit vector, the probe index, the successor table, a partitioned counter's
 *     count view) is complete before it is published: a later call sees it whole, whichever stream it names.
 *   - one MUTABLE object (a counter; a set while it is being built; a chain) is driven from one stream at a time, unless
 *     an entry says otherwise: a caller that moves it to another stream orders the two streams itself (an event, or a
 *     synchronise).  The partition workspace of a BRX_COUNT_SORTED counter and a chain's workspace have no ordering of
 *     their own beyond this rule.  A closed set is immutable and may be read on any number of streams at once.         */
/* same on device buffers, asynchronous on `stream` for bit-vector sets                          */
int brx_set_insert_batch_device(brx_set_t *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                uint64_t total_bases, void *stream);
/* Solid::set(kmer, value) -- host-side slow path (tests, csv input) src/set/pcon.rs:38      */
int brx_set_set(brx_set_t *set, uint64_t forward_kmer, bool value);
/* KmerSet::get                                                     src/set/pcon.rs:189-191 */
bool brx_set_get(const brx_set_t *set, uint64_t forward_kmer);
/* n independent KmerSet::get calls in one launch; out[i] = 0/1 */
int brx_set_get_batch(const brx_set_t *set, const uint64_t *forward_kmers, uint32_t n, uint8_t *out);
/* KmerSet::k                                                       src/set/pcon.rs:193-195 */
uint8_t brx_set_k(const brx_set_t *set);
int brx_set_device(const brx_set_t *set);
/* .solid writer ([k][bits]); len = 1 + 2^(2k-4) (at least 2)                               */
int brx_set_export_solid_bytes(const brx_set_t *set, uint8_t *buf, size_t cap, size_t *len);
int brx_set_popcount(const brx_set_t *set, uint64_t *n_set_bits);
/* 1 for a SPARSE set: k >= 21, where the 2^(2k-1)-bit vector (256 GiB at k = 21) does not fit next to the data.
 * Such a set holds its solid k-mers only as a key list and as the probe index (exact, overflowing lines chain
 * into the next line).  get / get_batch / popcount / count_finish[_into] / the correction entry points work;
 * entries that need the bit vector (.solid import/export, set, insert_batch, device_bits, extract/or_keys)
 * return BRX_ERR_UNSUPPORTED (such a set goes to disk as a key file: brx_set_save_fd / brx_set_load_fd).  Sets are built by the partitioned counter (k <= 21).                          */
int brx_set_sparse(const brx_set_t *set);
/* 0: the bit vector is in HBM and current; 1: LAZY -- a partitioned brx_set_count_finish[_into] listed the solid
 * hashes and left the 2^(2k-4)-byte vector unwritten (16 GiB at k = 19); it is materialised by the first entry
 * that needs it (export, device_bits, set, insert_batch, extract/or_keys, correction with a walking method);
 * get / get_batch / popcount / correction with One answer from the key list / probe index (BRX_LAZY_BITS=0
 * writes the vector at finish time as the reference does); 2: sparse set, no bit vector ever.                */
int brx_set_bits_state(const brx_set_t *set);
/* device view of the packed bit array (for RCCL all-gather / OR across ranks)              */
int brx_set_device_bits(const brx_set_t *set, void **d_bits, uint64_t *n_bytes);
/* sparse replication of the set: list the set bits of [first_hash, first_hash+n_hashes) (both
 * multiples of 32) as absolute bit indices, any order; OR a list of bit indices into a set      */
int brx_set_extract_keys_device(const brx_set_t *set, uint64_t first_hash, uint64_t n_hashes, uint64_t *d_out, uint64_t cap,
                                uint64_t *n_out, void *stream);
int brx_set_or_keys_device(brx_set_t *set, const uint64_t *d_keys, uint64_t n, void *stream);
/* ---- probe index: no counterpart in the reference (an HBM-locality copy of the same set) ------
 * KmerSet::get is one bit of a 2^(2k-1)-bit vector; the k-mers a read walks through hit unrelated
 * 64-byte lines.  The index stores the solid k-mers a second time in 64-byte lines addressed by the
 * k-mer's strand-symmetric minimizer, so that neighbouring k-mers of a read share a line.  It is exact
 * (full keys; a line that overflowed sends the probe back to the bitset) and only changes where
 * `get` reads.  The correction entry points build it on first use for 15 <= k <= 19 (BRX_INDEX=0
 * disables); every mutation of the bits through this ABI drops it.  m = minimizer length (odd, <= 15),
 * log2_lines = table size; 0 = automatic.                                                          */
int brx_set_index_build(brx_set_t *set, int m, int log2_lines, void *stream);
/* same, from a device list of the set's bit indices (e.g. the keys just exchanged between ranks)     */
int brx_set_index_build_from_keys_device(brx_set_t *set, const uint64_t *d_keys, uint64_t n, int m, int log2_lines,
                                         void *stream);
int brx_set_index_drop(brx_set_t *set);
/* the list of the set's bit indices (any order) when the builder produced one on the side (partitioned
 * brx_set_count_finish[_into]); *d_keys == NULL when there is none.  Valid until the set is mutated.
 * Lets the multi-GPU exchange ship the solid k-mers of a rank's range without scanning the bit vector.  */
int brx_set_keylist_device(const brx_set_t *set, void **d_keys, uint64_t *n, void *stream);
/* Three numbers that depend on the SET alone, not on what holds it (bit vector, solid-hash list, chained table):
 * out3[0] = members, out3[1] = sum of their hashes (canonical >> 1) mod 2^64, out3[2] = sum of the squares mod 2^64.
 * What the ranks of a multi-GPU job compare after the exchange (bench.py `checks.set_agree`): the reference has one
 * process and one set (src/main.rs:35-47); here every rank must end with the same one.                              */
int brx_set_fingerprint(const brx_set_t *set, uint64_t *out3, void *stream);
/* info8: [0] valid, [1] m, [2] log2_lines, [3] keys, [4] keys left to the bitset (overflow), [5] bytes,
 * [6] the correction entry points would use an index for this k, [7] a key list is attached          */
int brx_set_index_info(const brx_set_t *set, uint64_t *info8);
/* brx_set_get_batch answered through the index (+ bitset for overflowed lines); *n_fallback = probes
 * that needed the bitset                                                                             */
int brx_set_get_batch_indexed(const brx_set_t *set, const uint64_t *forward_kmers, uint32_t n, uint8_t *out,
                              uint64_t *n_fallback);
void brx_set_free(brx_set_t *set);

/* ---- coverage: which bases of a read the set supports.  No counterpart in the reference --------------------------
 * For a read s of n bytes and a set of k-mer length k:
 *   solid[i], 0 <= i <= n-k, is KmerSet::get (src/set/pcon.rs:189-191) of the forward k-mer s[i..i+k), every byte coded
 *     as nuc2bit codes it -- a byte that is not ACGT is a base like any other; n < k gives no k-mers;
 *   covered[j], 0 <= j < n, is true if some solid[i] holds with j-k+1 <= i <= j;
 *   a RUN is a maximal stretch of covered bases (at least k long);
 *   the MASKED form of a read has every letter (either case) in upper case where covered and in lower case where not;
 *     other bytes stay.  Lower-case letters have the same 2-bit codes, so masking never changes a k-mer;
 *   the SPLIT form with min_len is the runs of at least min_len bases (0 keeps every run), reads in order, the runs of
 *     a read in order of their start, each a piece of its own; a read without such a run yields nothing.
 * One probe per k-mer of the batch, 64 neighbouring positions per wave step, through whatever holds the set (bit
 * vector, key list + probe index, chained table): a cover call never mutates the set, never drops its index and never
 * materialises a lazy bit vector (brx_set_bits_state stays 1).  The probe index is built on first use like the
 * correction entries do.  Scratch comes from the device pool per call, so any number of host threads may cover
 * against one set on their own streams.  A read holds fewer than 2^32 - 16 bases.                                   */
#define BRX_COVER_SOLID_START 1u /* the k-mer that starts at this base is in the set */
#define BRX_COVER_COVERED 2u     /* the base lies inside at least one solid k-mer     */
typedef struct brx_cover_stats {
    uint32_t kmers;   /* max(n-k+1, 0)    */
    uint32_t solid;   /* sum of solid[]   */
    uint32_t covered; /* sum of covered[] */
    uint32_t runs;
} brx_cover_stats_t;
/* d_flags: one byte per base, laid out like d_bases (the two bits above); d_masked: the masked form, may alias d_bases;
 * d_stats: n_reads entries.  Any of the three may be NULL.  The work is enqueued on `stream`; the call returns after
 * its kernels have completed (its scratch goes back to the pool).                                                   */
int brx_set_cover_batch_device(const brx_set_t *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                               uint64_t total_bases, uint8_t *d_flags, uint8_t *d_masked, brx_cover_stats_t *d_stats,
                               void *stream);
/* same on host buffers (offsets[0] == 0); `masked` may alias `bases`                                                  */
int brx_set_cover_batch(const brx_set_t *set, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint8_t *flags,
                        uint8_t *masked, brx_cover_stats_t *stats);
/* split form.  Piece p is d_out[d_out_offsets[p] .. d_out_offsets[p+1]) (piece_cap + 1 offsets), bases
 * d_piece_start[p] .. of read d_piece_read[p] (either table may be NULL).  Bounds a caller can allocate by without a
 * retry: *out_total <= total_bases, *n_pieces <= n_reads + total_bases / (max(k, min_len, 1) + 1).  BRX_ERR_OVERFLOW
 * with the needed values in *n_pieces / *out_total (and nothing written) if piece_cap or out_cap is too small -- a call
 * with both 0 and NULL outputs asks for the sizes.  The order of the pieces is fixed by the definition, never by timing. */
int brx_set_cover_split_batch_device(const brx_set_t *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                     uint64_t total_bases, uint32_t min_len, uint8_t *d_out, uint64_t out_cap,
                                     uint64_t *d_out_offsets, uint32_t *d_piece_read, uint64_t *d_piece_start, uint32_t piece_cap,
                                     uint32_t *n_pieces, uint64_t *out_total, void *stream);
/* same on host buffers; the four outputs (*n_pieces + 1 offsets) are allocated by the library: release with brx_buf_free */
int brx_set_cover_split_batch(const brx_set_t *set, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint32_t min_len,
                              uint8_t **out_bases, uint64_t **out_offsets, uint32_t **piece_read, uint64_t **piece_start,
                              uint32_t *n_pieces);

/* ---- trusted stretches: the parts of a read worth counting.  No counterpart in the reference -----------------------
 * The reference counts every k-mer of every record, and nuc2bit gives every byte a 2-bit code: a stretch of N becomes a
 * homopolymer k-mer counted once per position, a k-mer over a Q2 base counts like one over Q40 bases.  That stays the
 * default; the entries below switch it off.  br_amd/trust.py states the definitions in numpy.
 * For a read s of n bytes, an optional quality string q of n bytes (Phred+33, the only encoding), a floor min_quality
 * (0..93) and acgt_only:
 *   letter[j]   s[j] is one of ACGTacgt;
 *   good[j]     min_quality == 0, or q is absent, or q[j] >= 33 + min_quality (a byte below 33 fails any floor above 0);
 *   trusted[j]  (letter[j] or not acgt_only) and good[j];
 *   a STRETCH is a maximal run of trusted bases;
 *   the SPLIT form with min_len is the stretches of at least max(min_len, 1) bases, reads in order, the stretches of a
 *     read in order of their start, each a piece of its own -- the shape of the coverage split form.  With min_len = k the
 *     k-mers of the pieces are exactly the k-mers of the read none of whose bases is untrusted; with min_quality == 0 and
 *     acgt_only == 0 every base is trusted and the split form is the batch itself, empty reads dropped.
 * The batch is cut by position (tiles of 1024 bases, a wave each); a lane takes 16 aligned bytes of bases and 16 of
 * qualities per step, nothing is probed, and trusted[] is recomputed by the second pass instead of being stored: 2 bytes
 * read per base and pass, at most 1 written.  Statistics are integer sums and depend on neither geometry nor timing.
 * Profile timers "trust" (work list, both passes, scans) and "trust_copy" (keep, layout, copy).                          */
typedef struct brx_trust_opts {
    uint8_t min_quality; /* 0..93; 0: no floor                                              */
    uint8_t acgt_only;   /* non-zero: a byte that is not ACGTacgt is untrusted              */
    uint16_t reserved;   /* 0                                                               */
    uint32_t min_len;    /* split form; the _fd entries below set it to k themselves        */
} brx_trust_opts_t;
typedef struct brx_trust_stats {
    uint32_t bases;       /* n                                                  */
    uint32_t non_acgt;    /* not letter[], whatever acgt_only says              */
    uint32_t low_quality; /* letter[] and not good[], whatever acgt_only says   */
    uint32_t pieces;      /* stretches of at least max(min_len, 1) bases        */
    uint32_t kept_bases;  /* their bases                                        */
} brx_trust_stats_t;
/* Split form of a device batch on `device`.  d_quals (may be NULL: no qualities) is laid out like d_bases.  Outputs and
 * bounds as for brx_set_cover_split_batch_device: *out_total <= total_bases, *n_pieces <= n_reads + total_bases /
 * (max(min_len, 1) + 1); BRX_ERR_OVERFLOW with the needed values in *n_pieces / *out_total, and nothing written (d_stats
 * included), if piece_cap or out_cap is too small -- a call with both 0 and NULL outputs asks for the sizes.  d_stats (may be
 * NULL): n_reads entries.  Follows the stream contract above: the inputs need only be ready in the order of `stream`, the
 * call returns after its kernels have completed, scratch comes from the pool per call, so any number of host threads may
 * call it at once.  BRX_ERR_ARG, the cause named: null opts / offsets / bases / n_pieces / out_total, min_quality > 93, a
 * batch too large for one call.                                                                                           */
int brx_trust_split_batch_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint32_t n_reads,
                                 uint64_t total_bases, const brx_trust_opts_t *opts, uint8_t *d_out, uint64_t out_cap,
                                 uint64_t *d_out_offsets, uint32_t *d_piece_read, uint64_t *d_piece_start, uint32_t piece_cap,
                                 brx_trust_stats_t *d_stats, uint32_t *n_pieces, uint64_t *out_total, int device, void *stream);
/* same on host buffers (offsets[0] == 0; quals may be NULL; stats may be NULL, else n_reads entries of the caller's); the
 * four outputs (*n_pieces + 1 offsets) are allocated by the library: release with brx_buf_free                             */
int brx_trust_split_batch(const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint32_t n_reads,
                          const brx_trust_opts_t *opts, uint8_t **out_bases, uint64_t **out_offsets, uint32_t **piece_read,
                          uint64_t **piece_start, brx_trust_stats_t *stats, uint32_t *n_pieces, int device);

/* ---- set build by counting: src/main.rs:72-115 -------------------------------------------
 * Counter::<u8>::new(k) -> count_fasta -> Solid::from_count(k, counts, abundance).
 * k must be odd (Fasta::kmer_size forces it, src/cli.rs:277-279).
 * strategy: BRX_COUNT_DENSE keeps the reference's 2^(2k-1)-byte u8 table in HBM (k <= 19: 128 GiB);
 * BRX_COUNT_SORTED radix-partitions the canonical hashes and counts them bucket by bucket (same
 * set, no table; k <= 21, its keys are 32 bits wide after the first digit);
 * BRX_COUNT_TABLE counts into a hash table in HBM -- the chained 64-byte-line table sparse sets are made of, 7 keys per
 * line, with one u32 counter per slot in an array beside the lines that stops being incremented at 255, so a count
 * reads as min(255, occurrences) whatever the input.  Any odd k from 5 to 31.  The table is kept at most about half
 * full: when the distinct k-mers so far plus the bases of the next batch no longer fit, a larger one is allocated and
 * the keys are moved with their counts (add_batch_device may synchronise `stream` for that); past the largest table,
 * 2^30 lines (64 GiB of lines + 32 GiB of counters, 7.5 G slots), add_batch returns BRX_ERR_NOMEM.  finish lists the
 * keys with count > abundance in one pass and leaves an ordinary closed set: sparse for k >= 21, with its bit vector
 * written for k <= 19.  device_counts, load_counts, clamp, l1_view, add_partitioned_device, brx_exchange_build_partitioned
 * and brx_exchange_reduce_counts return BRX_ERR_UNSUPPORTED for such a counter; across GPUs it goes through
 * brx_exchange_table_merge / _spectrum / _table_finish (below, "multi-GPU").  A MERGED counter holds the k-mers its rank
 * owns with the counts of the whole job: add_batch[_device] and a second merge return BRX_ERR_ARG until brx_counter_reset
 * reopens it; brx_counter_abundance_* and get_counts answer for the owned k-mers and 0 for all others (there is no
 * abundance query across ranks); spectrum, finish and table_info describe the owned share.
 * BRX_COUNT_AUTO = DENSE below 15, SORTED for 15 <= k <= 21, TABLE for 23 <= k <= 31.                              */
enum { BRX_COUNT_AUTO = 0, BRX_COUNT_DENSE = 1, BRX_COUNT_SORTED = 2, BRX_COUNT_TABLE = 3 };
int brx_set_count_begin(uint8_t k, int device, int strategy, brx_counter_t **out);
int brx_set_count_add_batch(brx_counter_t *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads);
int brx_set_count_add_batch_device(brx_counter_t *c, const uint8_t *d_bases, const uint64_t *d_offsets,
                                   uint32_t n_reads, uint64_t total_bases, void *stream);
/* solid iff count > abundance (strict; pinned by tests/data/raw.k11.a2.solid).  The counter
 * stays valid (finish may be called again with another abundance) until freed.             */
int brx_set_count_finish(brx_counter_t *c, uint8_t abundance, void *stream, brx_set_t **out);
/* same, into an existing set of the same k/device (no allocation; asynchronous on `stream`)  */
int brx_set_count_finish_into(brx_counter_t *c, uint8_t abundance, void *stream, brx_set_t *dst);
/* forget everything counted so far (Counter::new without re-allocating; async on `stream`)   */
int brx_counter_reset(brx_counter_t *c, void *stream);
/* 256-bin histogram of the counts = pcon::spectrum::Spectrum::from_count (src/main.rs:93):
 * hist256[v] = number of canonical k-mers seen exactly v times (255 = 255 or more, 0 = never).  Either
 * strategy (TABLE: bins 1..255 from the slot counters, bin 0 = 2^(2k-1) - distinct k-mers); the counter is left as it
 * was, so brx_set_count_finish with the chosen threshold follows.                                       */
int brx_counter_spectrum(brx_counter_t *c, uint64_t *hist256, void *stream);
/* dense strategy only: device view of the u8 table, for the RCCL reduction of SURVEY 8(e)   */
int brx_counter_device_counts(brx_counter_t *c, void **d_counts, uint64_t *n_bytes);
/* dense strategy only: overwrite counters [first, first + n) with counts computed elsewhere -- `br count`
 * (src/main.rs:59-70: pcon::counter::Counter::from_stream) hands a whole table over this way        */
int brx_counter_load_counts(brx_counter_t *c, uint64_t first, const uint8_t *counts, uint64_t n);
/* clamp every count to min(count, cap) in place (the exact-sum trick before an u8 all-reduce) */
int brx_counter_clamp(brx_counter_t *c, uint8_t cap, void *stream);
/* partitioned strategy, multi-GPU exchange (done on keys instead of the count vector):
 * after ONE add_batch the canonical hashes sit grouped by their first radix digit.  l1_view exposes
 * that layout (u32 keys with the digit stripped, u64 offsets[n_buckets+1]); a rank owns a contiguous
 * range of buckets, receives the other ranks' segments of that range and registers them with
 * add_partitioned (the memory stays the caller's until the counter is finished/reset).           */
int brx_counter_l1_view(brx_counter_t *c, void **d_keys, void **d_l1off, uint32_t *n_buckets, uint64_t *n_keys);
int brx_counter_add_partitioned_device(brx_counter_t *c, const uint32_t *d_keys, const uint64_t *d_l1off, uint64_t n_keys);
/* table strategy only: [0] log2(lines) of the table (0: none yet), [1] its minimizer length, [2] distinct k-mers counted
 * (read back from the device: synchronises `stream`), [3] most bytes of table held at once (both tables during a regrow) */
int brx_counter_table_info(brx_counter_t *c, uint64_t *info4, void *stream);
/* *world, *rank (rank may be NULL) the counter was merged over by brx_exchange_table_merge; *world = 0 for a counter that is
 * not merged (never merged, reset since, or of another strategy)                                                        */
int brx_counter_merge_state(brx_counter_t *c, int *world, int *rank);

/* ---- sliced counting: a job larger than one counting table, counted part by part (br_amd/parts.py) -----------------
 * A table counter sliced as (part, parts) counts exactly the k-mers with
 *     brx_exchange_table_owner(hash, parts) == part,   hash = canonical(kmer) >> 1
 * and ignores the rest, so `parts` sweeps over the same reads count every k-mer once, each sweep in a table sized for its
 * share.  The lists of the sweeps (brx_counts_from_counter) have disjoint keys; their BRX_COUNTOP_MAX is the job's list.
 *   set_slice    parts 1 .. 4096, part < parts (BRX_ERR_ARG otherwise); parts == 1: an ordinary counter again.  Only on a
 *                table counter that holds nothing -- new, or brx_counter_reset since -- BRX_ERR_ARG otherwise, the message
 *                naming what it holds; dense and partitioned counters: BRX_ERR_UNSUPPORTED.  The table an emptied counter
 *                still has is given back (waits for the reset's zeroing), so every slice sizes its own, and the peak of
 *                brx_counter_table_info starts again.  brx_counter_reset keeps the slice.
 *   answers      everything that reads the counter describes the slice: spectrum (bins 1..255 the slice's, bin 0 =
 *                2^(2k-1) - its keys), finish[_into], table_info, brx_counter_save_fd and brx_counts_from_counter (a slice's
 *                file is a valid count file), get_counts and the abundance entries (0 for the k-mers of other parts).
 *   refusals     brx_counter_load_fd into a sliced counter (a file's keys are not filtered) and brx_exchange_table_merge /
 *                _spectrum / _table_finish on one (a slice is not a rank's shard): BRX_ERR_ARG.
 *   sizing       an unsliced table is sized for "every base of the batch is a new key".  A sliced one, whenever that bound
 *                does not fit the table it has (or it has none), first counts the batch's k-mers of the part in a pass
 *                without the table -- one number back, one synchronisation of the stream -- and sizes for the keys known
 *                plus that number: the smallest 2^L lines with 7 * 2^L >= 3 * need, L >= 12.  A batch that holds nothing of
 *                the part makes no table.
 *   slice        *part, *parts; 0, 1 for a counter never sliced or of another strategy.
 *   slice_stats  cumulative since the last reset, all 0 for an unsliced counter (synchronises `stream`): [0] valid k-mers
 *                seen, [1] k-mers of the part, i.e. walked into the table, [2] wave trips into the walk, [3] waves launched
 *                by the sliced count kernel.  The surviving k-mers are compacted before the walk, so only full waves walk
 *                but for one last trip per wave: stats[2] <= stats[1] / 64 + stats[3].                                   */
int brx_counter_set_slice(brx_counter_t *c, uint32_t part, uint32_t parts);
int brx_counter_slice(brx_counter_t *c, uint32_t *part, uint32_t *parts);
int brx_counter_slice_stats(brx_counter_t *c, uint64_t *stats4, void *stream);
void brx_counter_free(brx_counter_t *c);

/* ---- abundance: how often the k-mers of a read were counted.  No counterpart in the reference ---------------------
 * For a read s of n bytes and a counter of k-mer length k:
 *   count[i], 0 <= i <= n-k, is the counter's value for the canonical k-mer of s[i..i+k): min(255, occurrences counted so
 *     far), 0 if the k-mer was never counted.  Every byte is coded as nuc2bit codes it -- a byte that is not ACGT is a
 *     base like any other, lower case equals upper case; n < k gives no k-mers;
 *   the PROFILE is one byte per base, laid out like `bases`: byte i of a read is count[i], the last k-1 bytes of a read
 *     (all bytes of a read shorter than k) are 0;
 *   the HISTOGRAM is 256 u32 per read: hist[v] = number of i with count[i] == v;
 *   the STATISTICS are brx_abund_stats_t, all fields 0 when kmers == 0.
 * Integer arithmetic throughout: no result depends on the launch geometry or on timing.  One lookup per k-mer of the
 * batch, 64 neighbouring positions per wave step, the batch cut by position like a cover call.  Dense (BRX_COUNT_DENSE)
 * and table (BRX_COUNT_TABLE) counters are served as they are; a partitioned one (BRX_COUNT_SORTED) holds sorted keys, no
 * counts that could be looked up, and returns BRX_ERR_UNSUPPORTED until brx_counter_lookup_prepare has built its count
 * view (below).  A counter that has counted nothing answers zeros.
 * The calls take the counter's lock, see everything added before them (also after the table has regrown) and leave
 * the counter as it was: brx_counter_spectrum and brx_set_count_finish with any threshold still follow.
 * A read holds fewer than 2^32 - 16 bases.                                                                             */
typedef struct brx_abund_stats {
    uint32_t kmers;  /* max(n-k+1, 0)                                                            */
    uint32_t absent; /* hist[0]                                                                  */
    uint32_t above;  /* number of i with count[i] > abundance (strict, as in brx_set_count_finish) */
    uint32_t min;    /* of count[]                                                               */
    uint32_t median; /* the lower median: element (kmers-1)/2 of the sorted counts               */
    uint32_t max;
    uint64_t sum;    /* of count[]                                                               */
} brx_abund_stats_t;
/* d_profile: one byte per base; d_hist: n_reads rows of 256 u32; d_stats: n_reads entries.  Any of the three may be
 * NULL.  The work is enqueued on `stream`; the call returns after its kernels have completed (its scratch goes back to
 * the pool).  n_reads == 0 or total_bases == 0 launches nothing.                                                        */
int brx_counter_abundance_batch_device(brx_counter_t *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                       uint64_t total_bases, uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist,
                                       brx_abund_stats_t *d_stats, void *stream);
/* same on host buffers (offsets[0] == 0)                                                                                */
int brx_counter_abundance_batch(brx_counter_t *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                uint8_t abundance, uint8_t *profile, uint32_t *hist, brx_abund_stats_t *stats);
/* brx_set_get_batch's twin: out[i] = the count of the canonical form of forward_kmers[i] (low 2k bits)                  */
int brx_counter_get_counts(brx_counter_t *c, const uint64_t *forward_kmers, uint32_t n, uint8_t *out);
/* The count view of a partitioned counter.  prepare sends everything counted so far -- every batch, segments registered
 * with add_partitioned_device included -- through the radix levels the spectrum takes, then rewrites every last-level
 * bucket (4096 consecutive hashes) in place: its distinct keys sorted, min(255, count) in a byte array beside them (one
 * byte per counted k-mer, the only memory the view adds).  A lookup is then two neighbouring bucket offsets and a binary
 * search of at most 12 steps.  prepare returns after `stream` has been synchronised; on a dense or a table counter it
 * does nothing and returns BRX_OK.  The view holds until the counter is next used for anything that touches its batches or
 * the partition workspace: add_batch[_device], add_partitioned_device, finish / finish_into, spectrum, reset, l1_view
 * and the brx_exchange_* entries each drop it first, and abundance / get_counts refuse again until the next prepare
 * (prepare after the threshold is chosen and the set finished).  The counter itself is left as it was: spectrum and
 * finish with any threshold still follow and give what they gave before.  brx_counter_save_fd (key files, below) reads
 * the view too -- it is the count file in the file's order -- needs it like a lookup does, and leaves it valid.
 * state: *state = 1 if abundance / get_counts would answer (always for dense / table), 0 if they would refuse.
 * drop: frees the view's count array; state 0 for a partitioned counter, nothing to do for the others.
 * All three take the counter's lock.                                                                                    */
int brx_counter_lookup_prepare(brx_counter_t *c, void *stream);
int brx_counter_lookup_state(brx_counter_t *c, int *state);
int brx_counter_lookup_drop(brx_counter_t *c);

/* ---- key files: k-mer counts and solid sets on disk at any odd k.  No counterpart in the reference ----------------------
 * The reference keeps a set as a .solid file -- the 2^(2k-1)-bit vector, 256 GiB at k = 21 -- and counts as pcon's table of
 * 2^(2k-1) bytes.  A KEY FILE holds the sorted keys (canonical k-mer >> 1, the bit index every key list carries), optionally
 * with one count byte each, for odd k from 5 to 31: a 32-byte header (magic "BRXKMERS", version, k, flags, floor, 256 keys per
 * block, number of keys, sum of the keys mod 2^64 = brx_set_fingerprint's out3[1]) and blocks of 256 keys -- first key, a
 * width byte, the differences to the key before minus one packed at that width, the count bytes.  br_amd/keyfile.py states
 * the format in numpy; the encoding is canonical, so equal contents give equal bytes.  Listing, sorting, packing and
 * unpacking run on the GPU (profile timers "key_list", "key_sort", "key_pack", "key_unpack", then the existing "tab_merge" /
 * "index_insert"); the file passes through two page-locked pieces of BRX_KEYFILE_SLICE_KB KiB (default 8192), never through
 * one host allocation of its size.  Descriptors are read and written sequentially, without seeks: a pipe to or from a
 * compressor works, as with brx_count_fasta_fd.  A malformed stream is BRX_ERR_FORMAT with a message naming the cause (wrong
 * magic / version / block size, k even or out of range, a key >= 2^(2k-1), a count of 0 or below the floor, blocks out of
 * order, a key sum that does not match, a truncated stream, trailing bytes); an I/O error is BRX_ERR_ARG.
 * stats8 (may be NULL): [0] keys, [1] file bytes, [2] blocks, [3] largest width, [4] ns listing + sorting (load: merging
 * into the table / building the set), [5] ns packing or unpacking, [6] ns reading or writing the fd, [7] ns wall.
 *
 * Stable LSD radix sort of n keys by their low key_bits bits (1..64; higher bits are ignored and carried along), 8-bit
 * digits, ceil(key_bits / 8) passes; d_payload (may be NULL) holds one byte per key that moves with it.  Every pass is a
 * histogram, a scan and a scatter in launches of their own: no workgroup waits for another.  Scratch (a second key and
 * payload array, n / 2 bytes of histograms) comes from the device pool; returns after `stream` has been synchronised.    */
int brx_sort_keys_device(uint64_t *d_keys, uint8_t *d_payload /* may be NULL */, uint64_t n, uint32_t key_bits, void *stream);
/* The count file of a BRX_COUNT_TABLE counter: every k-mer with min(255, count) >= max(min_count, 1, the counter's floor),
 * with that count.  The counter is only read: spectrum, finish, abundance and get_counts answer afterwards what they did
 * before.  A partitioned counter (BRX_COUNT_SORTED, odd k from 7) saves its COUNT VIEW: read bucket by bucket the view is
 * the file's content in the file's order, so the entries with count >= max(min_count, 1) are compacted in place order --
 * a count, a scan and a write under "key_list", nothing under "key_sort" -- and packed ([4] of stats8: ns of the
 * compaction; such a counter is never floored; the same bytes as the table counter's file of the same reads).  The save
 * needs the view and never builds it: without one it returns BRX_ERR_UNSUPPORTED and names brx_counter_lookup_prepare.  It
 * only reads the view and leaves it: brx_counter_lookup_state stays 1, and abundance, get_counts, spectrum and finish answer
 * what they answered before.  A counter that counted nothing writes the header alone, counts flag set, from either
 * strategy.  Dense counters, and a counter merged across ranks (brx_counter_merge_state world != 0), return
 * BRX_ERR_UNSUPPORTED.  Takes the counter's lock and works on the counter's own stream.                                    */
int brx_counter_save_fd(brx_counter_t *c, uint8_t min_count /* 0 means 1 */, int out_fd, uint64_t *stats8);
/* ADDS the counts of a count file to a BRX_COUNT_TABLE counter of the same k (BRX_ERR_ARG otherwise): the table is regrown
 * for the k-mers it holds plus the file's, counts add and saturate at 255 -- loading the files of shards counted separately
 * gives the counter of all their reads, as brx_exchange_table_merge does across GPUs.  A set file (no counts) is
 * BRX_ERR_FORMAT; dense, partitioned (it holds occurrences, not counts to add to) and merged counters are
 * BRX_ERR_UNSUPPORTED.  A file saved with min_count f > 1 no longer knows the
 * k-mers seen fewer than f times: it loads only into an EMPTY counter (BRX_ERR_ARG otherwise), which is then FLOORED at f
 * until brx_counter_reset -- brx_set_count_finish[_into] with abundance < f - 1 (the set would miss members),
 * add_batch[_device] and a further load return BRX_ERR_ARG, spectrum bins 1..f-1 read 0, a save writes floor max(f,
 * min_count).  Files with floor 1 merge freely.  A load that fails once the stream is being read (BRX_ERR_FORMAT, I/O,
 * memory) leaves the counter RESET -- empty, floor 1, usable -- and says so in the message, never half loaded; an argument
 * fault (k, floor) leaves it as it was.                                                                                    */
int brx_counter_load_fd(brx_counter_t *c, int in_fd, uint64_t *stats8);
/* *floor = f for a counter floored by brx_counter_load_fd, 1 otherwise (any strategy)                                     */
int brx_counter_floor(brx_counter_t *c, uint8_t *floor);
/* The set file (keys, no counts, floor 0) of any set of odd 5 <= k <= 31, whatever holds it: a valid key list is used as it
 * is, a sparse set built by insertion lists the lines of its table, a bit vector its bits; the keys are sorted on the way.
 * The set is only read: a lazy bit vector stays lazy (brx_set_bits_state unchanged), the probe index stays.                */
int brx_set_save_fd(const brx_set_t *set, int out_fd, uint64_t *stats8);
/* A new closed set on `device` from a key file of either kind (the counts of a count file are checked and ignored: every key
 * listed is a member), k from the header.  k >= 21: a sparse set, its key list attached and its chained probe index built;
 * k <= 19: the key list attached as after a counted finish (k >= 15) and the bit vector written.  get, get_batch,
 * popcount, fingerprint, .solid export (k <= 19), cover and correction answer as for the set that was saved.               */
int brx_set_load_fd(int in_fd, int device, brx_set_t **out, uint64_t *stats8);

/* ---- set algebra: union, intersection, difference of solid sets at any odd k.  No counterpart in the reference -------------
 * br_amd/setops.py states the operations in numpy.  The hot path is a merge of two strictly ascending lists of u64 keys by
 * merge path (br_amd/csrc/brx_setops.hip): tiles of 2048 positions of the merged sequence, their borders found by a binary
 * search on the diagonal (ties: A first), both pieces in LDS with one key of halo each side, 8 keys per thread merged
 * serially.  Whether a key is in the other list is read off its neighbour there, so no thread or tile asks another.  Pass 1
 * counts the kept keys per tile, sums |A n B| and checks that both lists ascend strictly; a scan turns the counts into
 * offsets; pass 2 merges again, compacts in LDS and writes whole runs.  One profile timer, "set_merge".                     */
#define BRX_SETOP_UNION 0
#define BRX_SETOP_INTERSECT 1
#define BRX_SETOP_DIFFERENCE 2 /* A minus B */
#define BRX_SETOP_SYMDIFF 3
/* The raw operation, the counterpart of brx_sort_keys_device: d_a[0 .. na) and d_b[0 .. nb), each strictly ascending (either
 * may be empty, the two may be the same array), combined by `op` into d_out[0 .. *n_out), strictly ascending.  The inputs are
 * read in the order of `stream`; returns after `stream` has been synchronised.  sizes3 (may be NULL) receives |A|, |B|,
 * |A n B|.  d_out == NULL with cap == 0 asks for *n_out and sizes3 only.  A cap smaller than the result is BRX_ERR_ARG with
 * *n_out set to what is needed; unordered or repeated keys in an input, a bad op and a d_out that overlaps an input are
 * BRX_ERR_ARG with *n_out = 0; d_out is untouched in all these cases.  Scratch (two u64 per tile) comes from the device pool.  */
int brx_keys_combine_device(const uint64_t *d_a, uint64_t na, const uint64_t *d_b, uint64_t nb, int op, uint64_t *d_out,
                            uint64_t cap, uint64_t *n_out, uint64_t *sizes3 /* may be NULL */, void *stream);
/* A new closed set on the operands' device: the keys of both are listed and sorted as brx_set_save_fd does (a key list that
 * came from brx_set_load_fd or from this call is known to be in order and is not sorted again, until something rewrites or
 * drops it), merged, and the result is exactly the set
 * brx_set_load_fd makes from those keys -- k >= 21: sparse, key list attached, chained index built; k <= 19: the bit vector
 * written, the key list kept for k >= 15; an empty result is a valid empty set.  Both sets must have the same k and device
 * (BRX_ERR_ARG, the message names both), odd k from 5 to 31 (BRX_ERR_UNSUPPORTED otherwise), and may be held in any form;
 * a == b is allowed.  Both are only read: a lazy bit vector stays lazy, index and key list stay.  The call works on a stream of
 * its own and returns complete (a freshly created object, see "streams"); like brx_set_save_fd it is a host-path READER of
 * its operands and does not wait for a caller's non-blocking stream that still writes them.
 * stats8 (may be NULL): [0] |A|, [1] |B|, [2] |A n B|, [3] |result|, [4] ns listing + sorting, [5] ns merging, [6] ns
 * building the set, [7] ns wall.                                                                                             */
int brx_set_combine(const brx_set_t *a, const brx_set_t *b, int op, brx_set_t **out, uint64_t *stats8);
/* sizes3 = |A|, |B|, |A n B| of two sets under the same rules: listing, sorting and pass 1 alone, nothing is built          */
int brx_set_compare(const brx_set_t *a, const brx_set_t *b, uint64_t *sizes3);

/* ---- count lists: add, subtract, min, max and threshold count files without a table.  No counterpart in the reference -------
 * What set algebra is for sets, for counts.  A COUNT LIST is the content of a count file on one device: n keys (canonical
 * k-mer >> 1), strictly ascending, and one count byte each, every count >= the list's FLOOR >= 1 (the smallest count that was
 * kept; k-mers seen fewer times are unknown, as in a count file).  br_amd/countops.py states the operations in numpy.  With
 * ca, cb the counts of a key in A and in B (0 when absent):
 *     BRX_COUNTOP_ADD   min(255, ca + cb)   every key of either list
 *     BRX_COUNTOP_MAX   max(ca, cb)         every key of either list
 *     BRX_COUNTOP_MIN   min(ca, cb)         the keys of both
 *     BRX_COUNTOP_SUB   ca - cb             the keys with ca > cb; a key of B alone never appears
 * and a key whose result lies below min_count (0 means 1) is dropped.  Counts are bytes as they are: 255 means "255 or
 * more", so a difference from or by a saturated count is a bound, not a value.
 * The hot path (br_amd/csrc/brx_setops.hip) is set algebra's merge path with a count byte riding along: the same tiles of
 * 2048 merged positions, the same border search, key pieces in LDS with one key of halo each side, 8 positions per thread;
 * the count pieces lie beside the keys, B's with one count of halo behind it, because an equal pair is decided where A's key
 * is taken and B's key of the pair yields nothing.  Whether a key is kept depends on the counts, so pass 1 merges the counts
 * too; it also checks that both key lists ascend strictly and that no input count is 0.  A scan, then pass 2 compacts keys
 * and counts in LDS and writes one run of each per tile; what pass 2 wrote must equal the scanned total.  One profile timer,
 * "count_merge"; the byte histogram of a list runs under "count_hist".                                                       */
#define BRX_COUNTOP_ADD 0
#define BRX_COUNTOP_MAX 1
#define BRX_COUNTOP_MIN 2
#define BRX_COUNTOP_SUB 3 /* A minus B */
/* The raw operation, the twin of brx_keys_combine_device with the same stream contract: (d_ka, d_ca)[0 .. na) and (d_kb,
 * d_cb)[0 .. nb) are read in the order of `stream`, the call returns after `stream` has been synchronised.  Either list may
 * be empty, A and B may be the same arrays.  d_cout may be NULL (keys only).  sizes3 (may be NULL) receives |A|, |B|, |A n B|.
 * d_kout == NULL with cap == 0 asks for *n_out and sizes3 only.  A cap smaller than the result is BRX_ERR_ARG with *n_out set
 * to what is needed; unordered or repeated keys, a 0 count in an input, a bad op and an output that overlaps an input (keys
 * against keys, counts against counts) are BRX_ERR_ARG with *n_out = 0; the outputs are untouched in all these cases.        */
int brx_counts_combine_device(const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                              uint64_t nb, int op, uint8_t min_count /* 0 means 1 */, uint64_t *d_kout,
                              uint8_t *d_cout /* may be NULL */, uint64_t cap, uint64_t *n_out, uint64_t *sizes3 /* may be NULL */,
                              void *stream);
/* The JOINT SPECTRUM of two lists: J[ca][cb] = the number of keys of A u B whose count bytes are ca in A and cb in B (0 where
 * the list does not hold the key), u64[65536] with row ca and column cb (br_amd/countops.py joint).  Counts are bytes as they
 * are: 255 means "255 or more".  Shared and private k-mers, completeness, a k-mer-based error rate and the copy-number plot are
 * sums over it (countops.compare_summary).  One pass of the merge above (timer "count_joint": split, the pass, the copy out):
 * it reads what pass 1 reads, checks what pass 1 checks and writes nothing per key.  The bins ca, cb < 64 are kept per block in
 * LDS (16 KB of u32 beside the pieces) and added to the table once per block -- and before a u32 bin could wrap; a thread folds
 * the equal pairs of its 8 positions and adds each distinct pair once; pairs outside the corner go straight to the table, one
 * global add each: a list made of large counts is slow, never wrong.
 * Measured on the bench's 1 Gbp at k = 25, two half-job lists of 366 M entries each (tools/count_compare_bench.py,
 * profiles/count_compare_bench.json; ms per Gbp, median of 5): "count_joint" 8.15, brx_counts_compare 8.74 wall, against 5.64
 * for split + pass 1 + scan of a size-only brx_counts_combine_device over the same lists: 1.45x, from the 16 KB of bins (three
 * workgroups per CU where pass 1 has four), not from the adds (DESIGN.md sections 4, 10).
 * The raw entry has brx_counts_combine_device's stream contract: the inputs are read in the order of `stream`, the call returns
 * after `stream` has been synchronised.  Either list may be empty, A and B may be the same arrays.  On success d_joint is
 * overwritten as a whole, J[0][0] = 0, and sizes3 (may be NULL) receives |A|, |B|, |A n B|.  Unordered or repeated keys, a 0
 * count in an input and a d_joint that overlaps an input are BRX_ERR_ARG with the cause named, and d_joint is untouched: the
 * table is accumulated in scratch of the device pool and copied on success.                                                  */
int brx_counts_joint_device(const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                            uint64_t nb, uint64_t *d_joint /* u64[65536], row ca, column cb */, uint64_t *sizes3 /* may be NULL */,
                            void *stream);
/* The object: an immutable count list on one device.  Every entry below is host-path: it works on a stream of its own and
 * returns complete; a list may be read by any number of host threads at once.
 * A list answers lookups (get_counts, abundance) once brx_counts_lookup_prepare has built its bucket directory, about n/2
 * bytes beside the list's 9n: see "lookups in a count list" below.
 * NOT supported: lists across ranks, lists of dense or merged counters, and turning a list back into a table counter other
 * than through its file.                                                                                                    */
typedef struct brx_counts brx_counts_t;
/* The list of a count file, any odd k from 5 to 31, floor from the header; the descriptor is read sequentially, never
 * sought.  Every malformed stream brx_counter_load_fd refuses is refused with the same status and message; a set file (no
 * counts) is BRX_ERR_FORMAT.  *out stays NULL on failure.  stats8 as for brx_counter_load_fd ([4] is 0: nothing is merged).  */
int brx_counts_load_fd(int in_fd, int device, brx_counts_t **out, uint64_t *stats8);
/* The list brx_counter_save_fd would write with this min_count: a table counter is listed and sorted, a partitioned one
 * hands over its count view (brx_counter_lookup_prepare first); dense and merged counters, and a partitioned counter without
 * a view, are BRX_ERR_UNSUPPORTED in the save's words.  Floor: max(the counter's floor, min_count, 1).  The counter is only
 * read; takes its lock and joins its stream as the save does.  stats8: [0] entries, [4] ns listing + sorting, [7] ns wall.    */
int brx_counts_from_counter(brx_counter_t *c, uint8_t min_count /* 0 means 1 */, brx_counts_t **out, uint64_t *stats8);
/* The count file of the list, the bytes of keyfile.encode(k, keys, counts, floor): a load followed by a save reproduces the
 * file.  min_count above the list's floor drops the smaller counts first (one compaction) and becomes the file's floor.
 * stats8 as for brx_counter_save_fd ([4]: ns of that compaction).                                                            */
int brx_counts_save_fd(const brx_counts_t *l, uint8_t min_count /* 0 means 1 */, int out_fd, uint64_t *stats8);
/* info4: [0] k, [1] entries, [2] floor, [3] device                                                                           */
int brx_counts_info(const brx_counts_t *l, uint64_t *info4);
/* the list's device arrays (u64 keys, u8 counts; both NULL for an empty list), valid until the list is freed; read only      */
int brx_counts_device(const brx_counts_t *l, void **d_keys, void **d_counts, uint64_t *n);
/* A new list, `a op b`.  Same k and device (BRX_ERR_ARG otherwise, the message names both); a == b is allowed; both are only
 * read.  Floors, with fa, fb the operands' (br_amd/countops.py result_floor states the same):
 *     MAX, MIN   the result's floor is max(fa, fb), and the result is exact from there up: a value at or above it needs
 *                the key present with that count in an operand (MAX) or in both (MIN);
 *     SUB        needs fb == 1 (BRX_ERR_ARG: the k-mers B no longer knows would be subtracted as 0); the floor is fa;
 *     ADD        needs fa == fb == 1 (BRX_ERR_ARG, as brx_counter_load_fd refuses it: two unknown parts could add up to a
 *                count that must be present).
 * Results below max(that floor, min_count) are dropped, and that maximum is the new list's floor.  The output arrays are
 * sized from pass 1 (9 bytes per entry); the peak is both operands plus the result.
 * stats8 (may be NULL): [0] |A|, [1] |B|, [2] |A n B|, [3] |result|, [4] 0, [5] ns merging, [6] 0, [7] ns wall.               */
int brx_counts_combine(const brx_counts_t *a, const brx_counts_t *b, int op, uint8_t min_count /* 0 means 1 */, brx_counts_t **out,
                       uint64_t *stats8);
/* Two lists side by side: joint65536 (host, u64[65536], row ca, column cb) receives their joint spectrum (above) with
 * J[0][0] = 2^(2k-1) - |A u B|, so that the row sums are brx_counts_spectrum of a and the column sums that of b.  Same k and
 * device (BRX_ERR_ARG otherwise, the message names both); a == b is allowed; both are only read; lookup directories are
 * ignored.  Floors are taken as they are and refuse nothing: a key a floored list does not hold falls in row or column 0,
 * which for a list of floor f > 1 means "fewer than f times, or never", and the rows (columns) 1 .. f - 1 are empty.
 * stats8 (may be NULL): [0] |A|, [1] |B|, [2] |A n B|, [3] |A u B|, [4] 0, [5] ns merging, [6] 0, [7] ns wall.               */
int brx_counts_compare(const brx_counts_t *a, const brx_counts_t *b, uint64_t *joint65536, uint64_t *stats8 /* may be NULL */);
/* hist256[v] = entries with count v for v >= 1 (bins below the floor are 0, as a floored counter reports them), hist256[0] =
 * 2^(2k-1) - entries: the 256 numbers brx_counter_spectrum gives a table counter that loaded the same file.                   */
int brx_counts_spectrum(const brx_counts_t *l, uint64_t *hist256);
/* The solid set: the keys with count > abundance (strict), exactly the set brx_set_load_fd makes from those keys (k >= 21:
 * sparse with its chained index; k <= 19: bits written, key list kept from k = 15; an empty result is a valid empty set).
 * abundance < floor - 1 is BRX_ERR_ARG, as for a floored counter.
 * stats8 (may be NULL): [0] entries, [1] kept, [2] 0, [3] 0, [4] ns selecting, [5] 0, [6] ns building the set, [7] ns wall.   */
int brx_counts_finish(const brx_counts_t *l, uint8_t abundance, brx_set_t **out, uint64_t *stats8);
void brx_counts_free(brx_counts_t *l);
/* Lookups in a count list.  A sorted key list with a count byte beside each key lacks only an entry point: the LOOKUP
 * DIRECTORY.  For the list's n ascending keys (all below 2^(2k-1)) and 2^d buckets, shift = (2k-1) - d:
 *     dir[b] = number of keys < (b << shift), b = 0 .. 2^d (u64 offsets; dir[2^d] = n),
 * and a lookup of key x = canonical k-mer >> 1 reads dir[x >> shift] and dir[(x >> shift) + 1], searches keys[lo .. hi) and
 * reads the count byte beside the key it found.  The search takes a bucket of any size: a list that skews into one bucket is
 * slow, never wrong.  br_amd/countops.py states directory, choice of d and lookup in numpy.
 * prepare: log2_buckets < 0 chooses d as the smallest d >= 0 with 16 * 2^d >= n, capped at min(2k-1, 30) -- a mean of at most
 * 16 keys, one 128-byte request, per bucket, and about n/2 bytes of directory; a caller's own d is taken from 0 to that cap
 * (BRX_ERR_ARG above it).  One launch of its own (br_amd/csrc/brx_listlookup.hip, profile timer "list_dir"): a thread per
 * bucket border searches its lower bound, no workgroup waits for another.  Host-path like every list entry: a stream of its
 * own, complete on return.  The d already in place: nothing is done; another d: the directory is rebuilt.  An empty list
 * prepares to a directory of zeros and answers zeros.
 * info4: [0] 1 if lookups answer, [1] log2 buckets, [2] directory bytes, [3] keys in the fullest bucket (all 0 without a
 * directory).  directory: the device array and its 2^d + 1 entries, read only, valid until the next prepare / drop
 * (BRX_ERR_UNSUPPORTED without one).  drop: frees the directory; lookups refuse again.
 * prepare and drop take the list's lookup lock exclusively, the lookups below take it shared, so a prepared list is looked
 * up from any number of host threads at once; every other list entry ignores the directory and gives what it gave without
 * one.  brx_counts_combine's result has no directory.
 * The lookups are the twins of brx_counter_abundance_batch_device / _batch / brx_counter_get_counts ("abundance" above) with
 * the same definitions of profile, histogram and statistics, NULL outputs, n_reads == 0 and total_bases == 0, and for the
 * _device form the same stream contract (enqueued on `stream`, complete on return); the host forms work on a stream of their
 * own.  count[i] is the list's byte for the k-mer, 0 for a k-mer that is not listed: for a list of floor f > 1 a 0 means
 * "counted fewer than f times, or never".  Without a directory they return BRX_ERR_UNSUPPORTED and name
 * brx_counts_lookup_prepare: nothing builds it implicitly, as with the partitioned counter's count view.
 * Measured on the bench's 1 Gbp (tools/list_lookup_bench.py, profiles/list_lookup_bench.json; ms per Gbp, median of 5): at
 * k = 19 / 21 / 25, 582 / 625 / 698 M entries under 2^26 buckets (537 MB), list_dir 12.4; abundance statistics from the list
 * 105.3 / 105.8 / 107.1 against 17.1 / 18.1 / 30.7 from the table counter and 126.3 / 88.3 from the partitioned view (k = 19 /
 * 21).  A list is 3.5x to 6.2x slower to ask than the table: it is for the jobs that have no table (DESIGN.md sections 4, 10). */
int brx_counts_lookup_prepare(brx_counts_t *l, int log2_buckets /* < 0: chosen from n */);
int brx_counts_lookup_info(const brx_counts_t *l, uint64_t *info4);
int brx_counts_lookup_directory(const brx_counts_t *l, void **d_dir, uint64_t *entries);
int brx_counts_lookup_drop(brx_counts_t *l);
int brx_counts_abundance_batch_device(const brx_counts_t *l, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                      uint64_t total_bases, uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist,
                                      brx_abund_stats_t *d_stats, void *stream);
int brx_counts_abundance_batch(const brx_counts_t *l, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                               uint8_t abundance, uint8_t *profile, uint32_t *hist, brx_abund_stats_t *stats);
int brx_counts_get_counts(const brx_counts_t *l, const uint64_t *forward_kmers, uint32_t n, uint8_t *out);

/* ---- k-mer text: count lists to and from KMER<TAB>COUNT lines.  No counterpart in the reference ---------------------------
 * The form `jellyfish dump -c -t` and `kmc_tools transform ... dump` write, stated in numpy by br_amd/kmertext.py: per entry
 * the k-mer as k upper-case letters, one TAB, the count in decimal, '\n'; a line takes k + 3 + (count >= 10) + (count >= 100)
 * bytes.  Lines stand in ascending KEY order -- the list's order, not alphabetical.  The k-mer printed for key x, with c =
 * (x << 1) | (popcount(x) & 1) the canonical k-mer: BRX_TEXT_CANONICAL c itself, BRX_TEXT_LEX the alphabetically smaller
 * (A < C < G < T) of c and its reverse complement, the member Jellyfish -C and KMC print.  A count byte of 255 prints as 255.
 * Reading: lines end with '\n', one '\r' before it is dropped, the bytes behind the last '\n' are a line too, empty lines are
 * skipped.  A line is exactly k bytes of ACGTacgt, one or more of TAB / space, one or more decimal digits, nothing else;
 * the digits' value saturates at 255 and must not be 0; either strand may be listed, the key is canonical(k-mer) >> 1.
 * Kernels: br_amd/csrc/brx_kmertext.hip (profile timers "text_format", "text_parse", "text_runsum").                          */
#define BRX_TEXT_LEX 0
#define BRX_TEXT_CANONICAL 1
/* The raw entries, with brx_counts_combine_device's stream contract: the inputs are read in the order of `stream`, the call
 * returns after `stream` has been synchronised.  Scratch comes from the device pool.
 * format: the lines of entries (d_keys, d_counts)[0 .. n) in the order given into d_text, *bytes_out of them.  A cap smaller
 * than the text (or a NULL d_text) is BRX_ERR_ARG with *bytes_out set to what is needed and d_text untouched.  Keys are taken
 * modulo 2^(2k-1), counts as they are.
 * parse: ONE pair per non-empty line of d_text[0 .. bytes), in line order: (canonical key, min(255, value)).  It does NOT
 * sort and does NOT sum equal keys.  The text must end at a line end, or its end is the end of its last line.  A cap smaller
 * than the non-empty lines is BRX_ERR_ARG with *n_out set to their number.  On the first malformed line in text order:
 * BRX_ERR_FORMAT, *n_out = 0, err3 = { cause, line within this text from 0 (empty lines counted), column }, the cause worded
 * in brx_last_error; the outputs may have been written.  Causes: 1 a byte of the k-mer that is no base (column from 1), 2 /
 * 3 a k-mer shorter / longer than k (column: its bases), 4 no count, 5 a byte that is no digit (column from 1), 6 a count
 * of 0.  err3[0] == 0 otherwise.                                                                                              */
int brx_kmertext_format_device(int k, const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int strand, uint8_t *d_text, uint64_t cap,
                               uint64_t *bytes_out, void *stream);
int brx_kmertext_parse_device(const uint8_t *d_text, uint64_t bytes, int k, uint64_t *d_keys, uint8_t *d_counts, uint64_t cap, uint64_t *n_out,
                              uint64_t *err3, void *stream);
/* The host-path entries: a stream of their own, complete on return; the descriptor is written / read sequentially, never
 * sought, through the two page-locked pieces of BRX_KEYFILE_SLICE_KB KiB of the key files.
 * dump: the entries counted at least min_count times (as brx_counts_save_fd drops the others), slice by slice of
 * piece / (k + 6) entries: a slice is formatted while the one before it is written.  stats8 (may be NULL): [0] entries,
 * [1] text bytes, [2] slices, [4] ns compacting, [5] ns waiting for the device (formatting and copies not hidden behind the
 * fd), [6] ns fd, [7] ns wall.
 * import: the list a text states.  The host cuts every piece at its last '\n' and carries the rest in front of the next one;
 * a line longer than a piece is BRX_ERR_FORMAT.  k == 0 takes k from the first non-empty line: its bytes before the first
 * TAB / space (odd, 5..31; an empty text tells none: BRX_ERR_FORMAT).  The pairs are sorted (brx_sort_keys_device; skipped
 * when they never descend), equal keys -- a k-mer twice, or both strands listed apart -- ADD saturating at 255, then a sum
 * below `floor` is BRX_ERR_FORMAT, and `floor` becomes the list's floor.  A malformed line is BRX_ERR_FORMAT, the message
 * "k-mer text: line N: cause" with N counted from 1 over the whole stream, empty lines included.  On any error *out is NULL.
 * stats8 (may be NULL): [0] entries, [1] text bytes, [2] non-empty lines, [3] 1 if the sort ran, [4] ns sorting + summing,
 * [5] ns parsing, [6] ns fd, [7] ns wall.
 * from_arrays: the list of n host (key, count) pairs, checked on the device: keys strictly ascending and below 2^(2k-1),
 * counts >= floor; BRX_ERR_ARG names the first offending index.  n == 0 is the valid empty list.                             */
int brx_counts_dump_text_fd(const brx_counts_t *l, uint8_t min_count /* 0 means 1 */, int strand, int out_fd, uint64_t *stats8);
int brx_counts_import_text_fd(int in_fd, int k /* 0: from the first line */, uint8_t floor /* 0 means 1 */, int device,
                              brx_counts_t **out, uint64_t *stats8);
int brx_counts_from_arrays(int k, const uint64_t *keys, const uint8_t *counts, uint64_t n, uint8_t floor /* 0 means 1 */,
                           int device, brx_counts_t **out);

/* ---- multi-GPU: reads shard over the GPUs, the set is exchanged ONCE -----------------------------
 * The reference is one process with rayon threads over shared memory (src/main.rs:30-33, src/lib.rs:72-139); on N
 * GPUs every rank counts and later corrects its own block of the reads, and the single exchange step is the k-mer
 * counts.  It runs inside this library over RCCL (xGMI), so a host needs no collective library of its own:
 *   - one process per GPU: rank 0 calls brx_comm_unique_id and hands the 128 bytes to the other ranks by any means
 *     it has (file, socket, MPI, torch.distributed); every rank then calls brx_comm_init(id, world, rank, device);
 *   - one process driving several GPUs (the reference's shape): brx_comm_init_all(n, devices, comms[n]), then one
 *     host thread per GPU.
 * librccl is dlopen'ed by soname on first use (BRX_RCCL_PATH overrides); BRX_ERR_UNSUPPORTED if it cannot be found. */
typedef struct brx_comm brx_comm_t;
#define BRX_COMM_ID_BYTES 128
int brx_comm_unique_id(uint8_t *id128);
int brx_comm_init(const uint8_t *id128, int world, int rank, int device, brx_comm_t **out);
int brx_comm_init_all(int n_devices, const int *devices, brx_comm_t **out /* n_devices handles */);
int brx_comm_info(const brx_comm_t *comm, int *world, int *rank, int *device);
/* `c` (partitioned strategy) has counted this rank's reads in ONE add_batch.  Every rank calls this once, together:
 * the canonical hashes go to the rank owning their first radix digit (all-to-all of u32 keys), the owner finishes its
 * digit range with `count > abundance`, and every owner's solid hashes go to everybody (all-gather of u64 lists).  On
 * return `dst` holds the solid set of ALL ranks' reads -- what the reference's all-reduce of the count vector followed
 * by Solid::from_count gives (src/main.rs:112-114) -- its probe index is built, and `c` is empty again.  k=19, 1 Gbp
 * per GPU: ~3.5 GB of keys + 0.15 GB of lists per rank over xGMI instead of 120 GB + 15 GB for the u8 vector.   */
int brx_exchange_build_partitioned(brx_comm_t *comm, brx_counter_t *c, uint8_t abundance, brx_set_t *dst, void *stream);
/* dense strategy, north_star's form: in-place all-reduce of the 2^(2k-1)-byte u8 table, exact for `count >
 * abundance` (counts are clamped to abundance+1 first; int32 slices once world*(abundance+1) > 255); the caller
 * then runs brx_set_count_finish[_into] on every rank.                                                          */
int brx_exchange_reduce_counts(brx_comm_t *comm, brx_counter_t *c, uint8_t abundance, void *stream);
/* The host-side arithmetic of brx_exchange_build_partitioned, a pure function (no GPU, no communicator): from the
 * `world` level-1 offset tables (each n_buckets+1 entries, non-decreasing from 0) it gives, for `rank`, the owner
 * bounds (world+1: rank r owns first digits [bound[r], bound[r+1]) = [r*n_buckets/world, ...)), the keys it sends to
 * and receives from every rank, optionally the per-source segment tables (world x (n_buckets+1): the source's table
 * clamped to the owned range and rebased to the received segment) and the largest single message of the job (what
 * fixes the number of capped rounds on every rank alike).  Exposed so that hosts and tests can check the layout for
 * any world size; there is no reference counterpart (one process, src/main.rs:30-33).                            */
int brx_exchange_plan(const uint64_t *tables, int world, uint32_t n_buckets, int rank, uint32_t *bound, uint64_t *send_counts,
                      uint64_t *recv_counts, uint64_t *seg /* may be NULL */, uint64_t *largest_message /* may be NULL */);
/* ---- counted sets across GPUs at any odd k up to 31: counting tables merged by owner -----------------------------------
 * Every rank counts its shard into a BRX_COUNT_TABLE counter (any number of batches, none included), then all ranks make
 * the three calls below together, in this order; spectrum and finish may be repeated (another threshold) on the merged
 * counter.  Argument faults and local failures travel through a status exchange, so that all ranks return together.
 *
 * owner: the rank that sums a k-mer's counts.  hash = canonical k-mer >> 1 (the bit index every key list carries);
 *   owner = ((((hash * 0x9E3779B97F4A7C15) mod 2^64) >> 32) * world) >> 32.  A pure function (no GPU, no communicator);
 *   BRX_ERR_ARG for world < 1 or NULL pointers.                                                                         */
int brx_exchange_table_owner(const uint64_t *hashes, uint64_t n, int world, uint32_t *owner_out);
/* merge: every entry of the rank's table goes to its owner as a (u64 key, u8 count) pair -- 9 bytes per distinct k-mer,
 * (world-1)/world of them over the links, in rounds whose messages stay under BRX_A2A_CHUNK x 4 bytes -- and the owner
 * builds a fresh table with the sums.  On return `c` is MERGED: it holds exactly the k-mers this rank owns, each with
 * min(255, sum over all ranks of the rank's count) (exact: min(255, sum of min(255, c_i)) = min(255, sum of c_i)).  The old
 * table is freed before the new one is made: the peak is old table + 9 B per entry, then send + receive arrays + new table.
 * If anything fails once the table has been taken apart the error is returned and `c` is left EMPTY (as after reset).     */
int brx_exchange_table_merge(brx_comm_t *comm, brx_counter_t *c, void *stream);
/* the job's spectrum from merged counters: every rank gets the same 256 numbers, what brx_counter_spectrum gives one
 * process that counted all the reads (the ranks' bins 1..255 all-gathered and summed, bin 0 = 2^(2k-1) - the rest)      */
int brx_exchange_spectrum(brx_comm_t *comm, brx_counter_t *c, uint64_t *hist256, void *stream);
/* the job's solid set (count > abundance) from merged counters into `dst` on every rank: the owner lists its solid k-mers
 * (and writes their bits when k <= 19), the lists go to everybody and are ORed into the bit vector / built into the probe
 * index, as build_partitioned does.  `c` stays merged and untouched.                                                    */
int brx_exchange_table_finish(brx_comm_t *comm, brx_counter_t *c, uint8_t abundance, brx_set_t *dst, void *stream);
/* last build_partitioned: [0] key bytes sent, [1] received, [2] keys counted by this owner, [3] its solid k-mers,
 * [4] solid k-mers of the job, [5] all-to-all us, [6] whole call us, [7] largest single message (keys).
 * After table_merge: [0] entry bytes sent over links, [1] received, [2] entries merged here, [3] = [4] = 0, [5] all-to-all
 * us, [6] whole call us, [7] largest single message (entries); table_finish then sets [3] and [4] and leaves the rest.    */
int brx_comm_last_stats(const brx_comm_t *comm, uint64_t *stats8);
void brx_comm_free(brx_comm_t *comm);

/* ---- correction: src/lib.rs:22-139 (run_correction) + src/correct/mod.rs:44-108 ----------
 * brx_chain_new = build_methods (order kept, duplicates allowed).  two_side=true means the
 * -s flag was given, i.e. the reverse pass is SKIPPED (src/lib.rs:48,110).                  */
int brx_chain_new(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, bool two_side,
                  brx_chain_t **out);
/* The second scan of a chain (no counterpart in the reference beyond NONE / REVERSE).  With fwd(x) = mn(..m1(x)), every
 * mi one Corrector::correct (src/correct/mod.rs:44-108), and rc(x) = the bytes of x in reverse order with A<->T, C<->G,
 * a<->t, c<->g exchanged and every other byte left as it is, a record s becomes
 *   BRX_PASS_NONE     fwd(s)                         (-s, two_side = true)
 *   BRX_PASS_REVERSE  rev(fwd(rev(fwd(s))))          (the reference's default, src/lib.rs:48-55,111: reversed, NOT complemented)
 *   BRX_PASS_REVCOMP  rc(fwd(rc(fwd(s))))            (the second scan runs along the other strand: it meets as many solid
 *                                                     k-mers as the first and attacks the right edge of every weak stretch)
 * brx_chain_new(.., two_side, ..) is brx_chain_new_pass with NONE / REVERSE.  brx_chain_last_stats[3] counts the fixes of
 * both scans.  brx_chain_second_pass returns the mode (negative brx_status for a null chain).                            */
enum { BRX_PASS_NONE = 0, BRX_PASS_REVERSE = 1, BRX_PASS_REVCOMP = 2 };
int brx_chain_new_pass(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, int second_pass,
                       brx_chain_t **out);
int brx_chain_second_pass(const brx_chain_t *chain);
/* rc() of every read of a batch, read r to d_out[d_offsets[r] .. d_offsets[r+1]) (same layout; d_out must not alias
 * d_bases; a read holds fewer than 2^32 - 1 bases).  Enqueued on `stream` of the current device; returns after the kernel
 * has completed.  Profile timers: "strand" (this entry and the step between the scans) and "strand_compact" (the
 * compaction of a REVCOMP chain); a chain in another mode starts neither.                                               */
int brx_revcomp_batch_device(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                             uint8_t *d_out, void *stream);
/* same on host buffers, through GPU `device`; `out` holds offsets[n_reads] bytes                                         */
int brx_revcomp_batch(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint8_t *out, int device);
/* one batch of records through the whole per-record body of run_correction
 * (src/lib.rs:42-55): every method in order, then (unless two_side) reverse, every method,
 * reverse back.  Output in input order.  *out_bases / *out_offsets are malloc'd by the
 * library; release with brx_buf_free.                                                       */
int brx_chain_correct_batch(brx_chain_t *chain, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                            uint8_t **out_bases, uint64_t **out_offsets);
/* The same batch, started and collected in two calls, so that ONE host thread can keep several chains of a set busy:
 * the next batch's upload runs under this one's kernels under the last one's download (a chain owns a stream and a
 * workspace; batches on different chains overlap, a chain takes one batch at a time).  `bases` / `offsets` must stay
 * valid until _wait returns; _wait blocks, returns what brx_chain_correct_batch would have returned and hands out the
 * same callee-allocated buffers.  This is the loop run_correction's 8192-record batches map to (src/lib.rs:84-132):
 * INTEGRATION.md shows it.  brx_chain_free waits for a batch still in flight.                                          */
int brx_chain_correct_batch_async(brx_chain_t *chain, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads);
int brx_chain_correct_batch_wait(brx_chain_t *chain, uint8_t **out_bases, uint64_t **out_offsets);
/* same on device buffers: d_out (capacity out_cap bytes) and d_out_offsets (n_reads+1) are
 * caller-allocated; *out_total receives the number of corrected bytes.  Returns
 * BRX_ERR_OVERFLOW (with *out_total = needed) if out_cap is too small.  The call returns
 * after its kernels have completed on `stream`.                                            */
int brx_chain_correct_batch_device(brx_chain_t *chain, const uint8_t *d_bases, const uint64_t *d_offsets,
                                   uint32_t n_reads, uint64_t total_bases, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *d_out_offsets, uint64_t *out_total, void *stream);
/* counters of the last batch: [0] scan rounds, [1] probes issued, [2] triggers, [3] fixes -- the fixes WRITTEN into the
 * reads that came back (Some(..) returns of correct_error, src/correct/mod.rs:75: the oracle's count), whereas
 * [0]-[2] count work done, speculative stretches included --,
 * [4] overflow retries, [5] reads that outgrew their output slot and [6] graph walks that outgrew the
 * visited list in the attempts that were redone; [7] the last lane-per-chunk pass (forward scan cut into units at
 * predictable states): units in bits 0-31, reads handed back to the group kernel in bits 32-55
 * (three predictions in a row missed, a list overflowed), and in bits 56-63 the unit records the replay found
 * unwritten (an invariant: always 0; the suites assert it); 0 = that form did not run                          */
int brx_chain_last_stats(const brx_chain_t *chain, uint64_t *stats8);
void brx_chain_free(brx_chain_t *chain);
void brx_buf_free(void *p);
/* Page-locked host memory for batch buffers.  brx_chain_correct_batch / brx_set_count_add_batch accept ANY host
 * pointer, but a batch in pageable memory is first copied into a page-locked block by the library (the DMA engines
 * read nothing else at full speed); a caller that fills buffers from brx_host_alloc -- the reference's
 * populate_buffer, src/lib.rs:168-188, is the natural place -- skips that copy.  The blocks are pooled; release with
 * brx_host_free (or brx_buf_free: the callee-allocated outputs of the batch entries are the same kind of block).      */
void *brx_host_alloc(size_t bytes);
void brx_host_free(void *p);
/* Device memory of the library is pooled too: blocks of 32 MiB and more are kept when a counter, set or chain is freed
 * (up to BRX_DEVPOOL_GB GiB per process, default 48; 0 = no pool) and reused by the next one -- the reference builds and
 * drops its 2^(2k-1)-byte counter table and its set once per run (src/main.rs:60-115), a host that runs job after job
 * would otherwise pay the driver's unmap / map of gigabytes every time.  brx_devpool_trim gives everything that is parked
 * back to the runtime (a host that needs the HBM for something else); brx_devpool_bytes says how much that is.            */
void brx_devpool_trim(void);
uint64_t brx_devpool_bytes(void);

/* ---- host pipelines over file descriptors ----------------------------------------
 * run_correction (src/lib.rs:22-139) for ONE input/output pair: FASTA records are parsed from in_fd (plain
 * text; decompress upstream), corrected by build_methods(methods) against `set` (reverse pass unless
 * two_side), and written to out_fd in input order as '>name[ description]' + the sequence wrapped at 80
 * columns (noodles' reader / writer conventions, restated; unpinned by the reference's tests).  Parsing, the
 * GPU (two chains on two streams, each worker also lays out the 80-column text of its batch) and writing run on
 * their own threads.  A malformed record ends the stream silently after the records before it (src/lib.rs:35).
 * max_batch_records 0 = default (batches of 32 MB of bases, BRX_PIPE_BATCH_MB); the batch size does not change
 * a byte of the output.
 * stats8: [0] records, [1] bases in, [2] bases out, [3] batches, [4..7] ns parsing / GPU + formatting (summed
 * over the workers) / writing / wall.                                                                        */
int brx_run_correction_fd(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, bool two_side, int in_fd,
                          int out_fd, uint32_t max_batch_records, uint64_t *stats8);
/* brx_run_correction_fd with an output form (no counterpart in the reference; "coverage" above has the definitions):
 *   BRX_OUT_MASK   the corrected records in their masked form: lower case where no solid k-mer covers the base;
 *   BRX_OUT_SPLIT  the covered runs of at least min_len bases of every corrected record, piece i (1-based, counted over
 *                  the pieces written) of record `name [description]` as `name_i [description]`; a record without such
 *                  a run writes nothing (what LoRDEC's trim-split does after its own correction).
 * The cover pass runs on the corrected batch on the device, between the correction and the layout of the text.
 * report_fd >= 0: a '#'-headed TSV, one line per input record in input order:
 *   name len_in kmers_in solid_in covered_in runs_in len_out kmers_out solid_out covered_out runs_out
 * (the _in columns cost one more cover pass, over the records as they came in; it runs only for a report or stats).
 * cover_totals8 (may be NULL; filled when stats != 0 or a report is written, else zeros): kmers, solid, covered, runs
 * summed over the INPUT records [0..3] and over the corrected records [4..7].
 * opts == NULL, or mode PLAIN without report and stats, is byte for byte brx_run_correction_fd and launches no cover
 * kernel (profile timer "cover").                                                                                   */
enum { BRX_OUT_PLAIN = 0, BRX_OUT_MASK = 1, BRX_OUT_SPLIT = 2 };
typedef struct brx_output_opts {
    uint32_t mode;    /* BRX_OUT_PLAIN / MASK / SPLIT */
    uint32_t min_len; /* split only */
    int report_fd;    /* -1: none */
    uint32_t stats;   /* non-zero: fill cover_totals8 (a report implies it) */
} brx_output_opts_t;
int brx_run_correction_fd_opts(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, bool two_side, int in_fd,
                               int out_fd, uint32_t max_batch_records, const brx_output_opts_t *opts, uint64_t *stats8,
                               uint64_t *cover_totals8);
/* brx_run_correction_fd_opts with the second-pass mode of its chains (BRX_PASS_*; two_side false / true = REVERSE / NONE).
 * Mask, split, report and totals work on the result as before.                                                         */
int brx_run_correction_fd_pass(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, int second_pass, int in_fd,
                               int out_fd, uint32_t max_batch_records, const brx_output_opts_t *opts, uint64_t *stats8,
                               uint64_t *cover_totals8);
/* Counter::count_fasta(reader, record_buffer) (src/main.rs:73-78): counts every record of the FASTA stream */
int brx_count_fasta_fd(brx_counter_t *c, int in_fd, uint32_t max_batch_records, uint64_t *stats8);
/* Pcon::from_fasta / Hash::from_fasta (src/set/pcon.rs:47-112, src/set/hash.rs:40-60): every record of the stream
 * inserted presence-only (`br solid -f fasta`, `br large-kmer -f fasta`)                                          */
int brx_set_insert_fasta_fd(brx_set_t *set, int in_fd, uint32_t max_batch_records, uint64_t *stats8);
/* The same two over FASTA or FASTQ, optionally through the trusted stretches ("trusted stretches" above; no counterpart
 * in the reference, whose FASTQ readers are src/set/pcon.rs:114-181).  FASTQ: records of four lines -- '@' + a non-empty
 * name that does not start with whitespace, the sequence, a line that starts with '+', qualities of the sequence's length;
 * trailing \r / \n are stripped, a missing final newline is fine, an empty sequence is a valid record, and the first
 * malformed or truncated record ends the stream silently after the records before it (br_amd/fasta.py
 * read_fastq_sequences states the same rules).  A record is never split between batches.
 * opts == NULL: every k-mer of every record, every byte a base -- with BRX_READS_FASTA that is brx_count_fasta_fd /
 * brx_set_insert_fasta_fd, same launches, same result.  opts != NULL: every batch is cut into its trusted stretches of at
 * least k bases on the device (opts->min_len is ignored: the entries set it to k) and the pieces are counted / inserted;
 * FASTA has no qualities, so only acgt_only can bite there.
 * trust_totals8 (may be NULL): bases, non_acgt, low_quality, pieces, kept_bases, k-mers counted, 0, 0 -- summed over the
 * stream; with opts == NULL nothing is classified: non_acgt and low_quality are 0, pieces = the records of at least k bases,
 * kept_bases = their bases.  BRX_ERR_ARG for a format other than the two and for min_quality > 93, before anything is read. */
enum { BRX_READS_FASTA = 0, BRX_READS_FASTQ = 1 };
int brx_count_reads_fd(brx_counter_t *c, int in_fd, int format, uint32_t max_batch_records, const brx_trust_opts_t *opts,
                       uint64_t *stats8, uint64_t *trust_totals8);
int brx_set_insert_reads_fd(brx_set_t *set, int in_fd, int format, uint32_t max_batch_records, const brx_trust_opts_t *opts,
                            uint64_t *stats8, uint64_t *trust_totals8);

/* ---- synthetic reads: deterministic, identical on host and device ----------
 * genome: i.i.d. uniform ACGT of length genome_len (seed); read r: window of read_len
 * reference bases at a uniform start, strand +/- with p=1/2, per-reference-base errors
 * sub/ins/del at the given rates (parts per 10 000).  Output offsets are fixed-stride
 * capacity slots compacted by the call; *total receives the number of bases.               */
typedef struct brx_synth {
    uint64_t seed;
    uint64_t genome_len;
    uint32_t read_len;
    uint32_t sub_e4, ins_e4, del_e4;
} brx_synth_t;
int brx_synth_genome_device(const brx_synth_t *cfg, int device, uint8_t *d_genome, void *stream);
int brx_synth_reads_device(const brx_synth_t *cfg, int device, const uint8_t *d_genome, uint64_t first_read,
                           uint32_t n_reads, uint8_t *d_bases, uint64_t bases_cap, uint64_t *d_offsets,
                           uint64_t *total, void *stream);
int brx_synth_genome_host(const brx_synth_t *cfg, uint8_t *genome);
int brx_synth_reads_host(const brx_synth_t *cfg, const uint8_t *genome, uint64_t first_read, uint32_t n_reads,
                         uint8_t *bases, uint64_t bases_cap, uint64_t *offsets, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* BRX_H */
