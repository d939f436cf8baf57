// Internal declarations shared by the translation units of libbrx.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <atomic>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/brx.h"
#include "brx_kmer.hpp"
#include "brx_devbuf.hpp"
#include "brx_setstate.hpp"
#include "brx_index.hpp"

namespace brx {

void set_error(const char *fmt, ...);

#define BRX_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            brx::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
            return (_e == hipErrorOutOfMemory) ? BRX_ERR_NOMEM : BRX_ERR_HIP;                      \
        }                                                                                          \
    } while (0)

#define BRX_TRY(expr)                                                                              \
    do {                                                                                           \
        int _s = (expr);                                                                           \
        if (_s != BRX_OK)                                                                          \
            return _s;                                                                             \
    } while (0)

// BRX_OK if `device` is a usable GPU and has been made current
int use_device(int device);
// What the batch entries refuse (brx_api.hip); `what` names the entry in the message.  check_batch_args: null bases or
// offsets for a batch that has some, bases in no reads.  check_offsets, host offsets only: they start at 0 and do not
// decrease, and a read holds fewer than 2^32 - 16 bases; strand_rule (brx_revcomp_batch): they may start anywhere -- the
// bytes in front of offsets[0] belong to no read -- and a read holds up to 2^32 - 2 bases.
int check_batch_args(const char *what, const void *bases, const uint64_t *offsets, uint32_t n_reads, uint64_t total_bases);
int check_offsets(const char *what, const uint64_t *offsets, uint32_t n_reads, bool strand_rule = false);
// pooled page-locked host memory (brx_api.hip): what brx_host_alloc and the callee-allocated outputs are made of
void *host_buf_acquire(size_t bytes);
void host_buf_release(void *p);
bool host_buf_is_pinned(const void *p);

// device memory through the block pool (brx_devpool.hip; dev_alloc / dev_free are declared in brx_devbuf.hpp)
void dev_pool_trim();
size_t dev_pool_bytes();

// zeroes memory of an object under construction and returns when that is done, so that the object can be used on any
// stream at once (a plain hipMemset of device memory is only enqueued on the null stream, and neither the caller's
// non-blocking streams nor the library's own wait for that one).  Synchronising the null stream also waits for whatever the
// host has queued on it and on its blocking streams: heavier than the memset needs, accepted in a constructor -- sets have
// no stream of their own to zero on.
inline hipError_t zero_now(void *p, size_t bytes)
{
    const hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}

// BRX_TRACE=1: synchronise `s` and print a time-stamped stage name on stderr (finding where a big job stalls)
void trace_stage(hipStream_t s, const char *what);

// ---- per-kernel HIP-event timers -----------------------------------------------------------
// Usage: { KernelTimer t("correct_pass", stream); launch<<<...,stream>>>(); }
// Events are recorded on the launch stream and resolved lazily by brx_profile_get.
class KernelTimer {
  public:
    KernelTimer(const char *name, hipStream_t s);
    ~KernelTimer();

  private:
    int slot_;
    hipStream_t s_;
    hipEvent_t start_, stop_;
    bool on_;
};

// unsigned value of an environment variable (brx_onelane.hip), read per call: the tests and fuzzers sweep these
uint32_t env_u32(const char *name, uint32_t dflt);
// BRX_READ_GRID: fewer blocks for the helper kernels whose blocks loop over reads, records, runs (so that a small batch
// takes a block through several of them); unset or 0: the kernel's own cap
inline uint32_t read_grid(uint64_t want, uint32_t cap)
{
    const uint32_t v = env_u32("BRX_READ_GRID", 0u);
    if (v && v < cap)
        cap = v;
    return want < cap ? (uint32_t)want : cap;
}

// number of 32-bit words of the bitset for a given k (at least 1)
inline uint64_t set_nbits(int k) { return 1ull << (2 * k - 1); }
inline uint64_t set_nwords(int k) { uint64_t b = set_nbits(k); return b < 32 ? 1 : b / 32; }
inline uint64_t set_nbytes_file(int k) { return (set_nbits(k) + 7) / 8; }

} // namespace brx

// A solid set.  Its keys can be held four ways at once; who holds them RIGHT NOW is set_holder's rule (brx_setstate.hpp),
// asked through set_keys below, and the flags are written through bits_mark / keylist_mark / index_mark alone.
// The reachable states, and the entry that leaves each:
//   bits     current   brx_set_new, a .solid stream, a dense or table finish (k <= 19), a partitioned finish at k outside the
//                      indexed range or under BRX_LAZY_BITS=0, key files and set algebra (set_build_from_keys), and any
//                      lazy set after ensure_bits
//            lazy      (bits_stale) the partitioned finish at indexed k <= 19: allocated, not written
//            sparse    k >= 21, BRX_FORCE_SPARSE: no vector at all
//   list     none      sets that never had one; every mutation of the bits (index_invalidate); a table built from a
//                      foreign list while there are no bits (brx_set_index_build_from_keys_device); insert into a sparse set
//            complete  a finish at indexed k, key files and set algebra at indexed k (those two: sorted); the empty list of
//                      a fresh sparse set
//            truncated the device counter passed the capacity: only the partitioned finish that also writes current bits
//                      (BRX_LAZY_BITS=0) sizes its list below the exact bound, so only current bits meet it
//   index    none      until something asks; after index_invalidate / brx_set_index_drop
//            accelerator  built while the bits were current (index_ensure, brx_set_index_build): overflowed lines defer to the bits
//            exact, closed  built while there were no bits: chained, answers alone; stays exact if the bits appear later
//            exact, open    brx_set_insert_batch on a sparse set: the table is the set, more can be added, no list
//   lazy or sparse x no complete list x no exact table holds no keys (SetHolder::None): brx_set_index_drop on a set whose
//   table was all it had gets there, and every enumerating entry refuses it in its own words.
struct brx_set {
    int k;
    int device;
    uint64_t nwords;   // u32 words
    brx::DevBuf<uint32_t> d_bits; // nwords, zero padded; empty for a sparse set
    bool sparse;
    bool bits_stale;
    bool idx_exact;          // the index was built with chaining (answers without the bit vector)
    bool idx_open;           // ... and k-mer by k-mer: more can be added
    // probe index over the same set (brx_index.hpp): built on demand, invalidated by every mutation
    // of the bits that goes through the ABI
    brx::DevBuf<uint64_t> d_lines; // 8 u64 per line
    uint64_t lines_alloc;    // lines allocated (the allocation also holds lines_alloc / 8 bytes of occupancy bits behind the lines)
    bool idx_linebits = false; // the occupancy bits are current (indexes built from a key list)
    uint32_t idx_log_lines;
    uint32_t idx_m;
    bool idx_valid;
    bool idx_declined;       // index_ensure looked at the set and found an index would not help
    // successor table beside the index (brx_onelane.hip): per line, one byte per slot -- for either orientation of the
    // slot's k-mer, whether it has exactly one solid successor and which.  Built on first use by a walking corrector,
    // stale whenever the index changes (idx_gen counts the changes).
    brx::DevBuf<uint64_t> d_succ;
    uint64_t succ_lines = 0;     // lines the table was allocated for
    uint64_t succ_gen = ~0ull;   // idx_gen it was built at
    uint64_t idx_gen = 0;
    uint64_t idx_keys, idx_overflow_keys;
    brx::DevBuf<uint64_t> d_keylist;             // (its cap(): entries)
    brx::DevBuf<unsigned long long> d_keylist_n; // device counter (may exceed the list's capacity: list truncated)
    bool keylist_valid;
    bool keylist_sorted = false; // the valid list is known to ascend strictly: listing it needs no sort
    std::mutex idx_mu;
};

namespace brx {
struct IdxView;
// (re)builds the index from a device list of keys (bit indices = canonical >> 1); m / log_lines 0 = auto
int index_build_from_keys(brx_set *set, const uint64_t *d_keys, uint64_t n, int m, int log_lines, hipStream_t s);
int index_insert_reads(brx_set *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                       hipStream_t s);
// presence-only insertion over the flat base stream (brx_partbuild.hip); table == nullptr: atomicOr into `bits`
int flat_presence_insert(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k,
                         uint32_t *bits, uint64_t *table, uint32_t line_shift, uint32_t m, unsigned long long *d_new, hipStream_t s);
// counting into a chained table with a u32 counter per slot (brx_partbuild.hip: flat_count_kernel)
int flat_table_count(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint64_t *table,
                     uint32_t *counts, uint32_t line_shift, uint32_t m, unsigned long long *d_new, hipStream_t s);
// the same for a sliced counter (flat_count_slice_kernel: the k-mers `part` of `parts` owns, compacted in LDS so that
// only full waves walk), and the sizing pass without the table (d_out2: k-mers of the part, valid k-mers)
int flat_table_count_slice(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint64_t *table,
                           uint32_t *counts, uint32_t line_shift, uint32_t m, uint32_t part, uint32_t parts, unsigned long long *d_new,
                           unsigned long long *d_stats4, hipStream_t s);
int flat_slice_census(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint32_t part,
                      uint32_t parts, unsigned long long *d_out2, hipStream_t s);
// sets of this k have no bit vector
inline bool sparse_k(int k) { return k >= 21; }
// the set must be probed through its (chained) index: it has no bit vector, or not right now
inline bool no_bits(const brx_set *set) { return set->sparse || set->bits_stale; }
// materialises a stale bit vector (BRX_ERR_UNSUPPORTED for a sparse set)
int ensure_bits(const brx_set *set, hipStream_t s, const char *what);
// builds the index from the bitset when the set has none (no-op for k outside the indexed range)
int index_ensure(const brx_set *set, hipStream_t s);
// the one place each group of flags is written.  keylist_mark: a list is in order only where its writer says so.
// bits_mark: the vector is written (or being written on the caller's stream) / allocated but unwritten.  index_mark: what
// a finished build leaves -- chained, open to more k-mers, occupancy bits filled.
inline void keylist_mark(brx_set *set, bool valid, bool sorted = false) { set->keylist_valid = valid; set->keylist_sorted = valid && sorted; }
inline void bits_mark(brx_set *set, bool current) { set->bits_stale = !current; }
inline void index_mark(brx_set *set, bool exact, bool open, bool linebits) { set->idx_exact = exact; set->idx_open = open; set->idx_linebits = linebits; set->idx_valid = true; set->idx_gen++; }
inline void index_invalidate(brx_set *set) { set->idx_valid = false; set->idx_declined = false; keylist_mark(set, false); }
// Who holds the keys, resolved (brx_index.hip): the holder and what to read it through.  set_keys takes idx_mu, reads the
// list's counter once -- one 8-byte readback on `s` and its synchronisation, only when a list is attached -- and asks
// set_holder; set_keys_locked is the same for a caller that holds idx_mu.  None is not an error here: each caller has
// its own words for it.  listed_n / list_cap are what the rule was asked with (0 / the buffer's entries without a list).
struct SetKeys {
    SetHolder holder = SetHolder::None;
    KeySource src;           // the holder, as a kernel enumerates it (brx_index.hpp); a list's n is src.n
    bool sorted = false;     // KeyList: known to ascend strictly
    uint64_t table_keys = 0; // Table: the keys it holds
    uint64_t listed_n = 0, list_cap = 0;
};
int set_keys(const brx_set *set, hipStream_t s, SetKeys *out);
int set_keys_locked(const brx_set *set, hipStream_t s, SetKeys *out);
// the number of keys, on `s` (brx_set.hip): the list's, the table's, or the popcount kernel's.  A set that holds no keys
// answers what its truncated list counted (0 without one), as brx_set_popcount always has.
int keys_count(const brx_set *set, const SetKeys &keys, hipStream_t s, uint64_t *n);
int set_count(const brx_set *set, hipStream_t s, uint64_t *n);
// the keys of a current bit vector into d_out (brx_set.hip): popcount, room for them and `spare` more (at least one entry),
// extract; returns after `s` has run them.  counted: the popcount where the caller has taken it already.  A lazy vector is
// materialised first, a sparse set refused (ensure_bits).
int keys_from_bits(const brx_set *set, hipStream_t s, DevBuf<uint64_t> &d_out, uint64_t *n_out, uint64_t spare = 0,
                   const uint64_t *counted = nullptr);
// every slot of a chained table that holds a key seen at least min_count times (counts == nullptr: every key), compacted
// into d_keys / d_cnts in no order, *d_n (zeroed by the caller) counting them past `cap` too (brx_keyfile.hip; timer "key_list")
int table_list(const uint64_t *lines, const uint32_t *counts, uint64_t n_entries, uint32_t min_count, uint64_t *d_keys, uint8_t *d_cnts,
               uint64_t cap, unsigned long long *d_n, hipStream_t s);
int index_auto_m(int k, uint64_t n_keys);
bool index_wanted(int k);
}

namespace brx { struct PartState; struct TabState; }

namespace brx {
// reverse complement of staged reads (brx_strand.hip; profile timers "strand" / "strand_compact"): into the other staging buffer, lengths
// carried over (a poisoned length stays poisoned), and into the compact output (compact_kernel's sibling)
void revcomp_stage(const uint8_t *stage_in, const uint32_t *lens_in, const uint64_t *d_offsets, uint32_t n_reads, uint32_t slack,
                   uint8_t *stage_out, uint32_t *lens_out, hipStream_t s);
void revcomp_compact(const uint8_t *stage, const uint32_t *lens, const uint64_t *d_offsets, uint32_t n_reads, uint32_t slack,
                     const uint64_t *d_out_offsets, uint8_t *d_out, hipStream_t s);
void revcomp_host(uint8_t *p, size_t n); // in place, on the host (the few reads redone outside their batch)
}

struct brx_counter {
    int k;
    int device;
    int strategy;
    // dense: u8 table packed in u32 words (2^(2k-1) bytes, padded to 32 B)
    brx::DevBuf<uint32_t> d_counts;
    uint64_t count_bytes;
    // partitioned strategy (brx_partbuild.hip)
    brx::PartState *part;
    brx::DevBuf<uint64_t> d_keys;
    uint64_t n_keys;
    // counting-table strategy (brx_counttable.hip)
    brx::TabState *tab = nullptr;
    hipStream_t stream; // owned, used by host-pointer entry points
    // what a stream-taking entry last enqueued on the caller's stream (include/brx.h "streams"): recorded by
    // counter_mark, waited for in counter_join by the stream a host-pointer entry works on, before it touches the counter
    hipEvent_t ev = nullptr;
    std::atomic<bool> ev_pending{false};
    std::mutex mu;
};

namespace brx {
inline hipError_t counter_mark(brx_counter *c, hipStream_t s)
{
    if (!c->ev || s == c->stream)
        return hipSuccess;
    const hipError_t e = hipEventRecord(c->ev, s);
    if (e == hipSuccess)
        c->ev_pending = true;
    return e;
}
// `on`: the stream the host-pointer entry works on -- the counter's own, or the null stream (brx_counter_load_counts)
inline hipError_t counter_join(brx_counter *c, hipStream_t on)
{
    if (!c->ev_pending.exchange(false))
        return hipSuccess;
    return hipStreamWaitEvent(on, c->ev, 0);
}
}

namespace brx {
// counting table of a BRX_COUNT_TABLE counter as a read-only lookup sees it (brx_counttable.hip)
void tab_view(const brx_counter *c, const uint64_t **lines, const uint32_t **counts, uint32_t *log_lines, uint32_t *m);
// The rank of a multi-GPU job that sums the counts of a k-mer (brx_exchange_table_merge): a multiplicative hash of the
// k-mer's bit index (canonical >> 1) spread over `world` by the top-bits product, so neighbouring hashes part.  ONE
// definition for the split kernel and for brx_exchange_table_owner; br_amd/dist.py table_owner states it in numpy.
__host__ __device__ inline uint32_t table_owner_of(uint64_t hash, uint32_t world)
{
    return (uint32_t)((((hash * 0x9E3779B97F4A7C15ull) >> 32) * (uint64_t)world) >> 32);
}
// The table side of that merge (brx_counttable.hip).  split: every entry of the table into two arrays the call allocates
// (keys u64 = bit indices, counts u8 = min(255, count)), grouped by owner, per_owner[r] entries for rank r in rank order;
// the table is freed, the arrays are the caller's (DevBuf::adopt them; both nullptr when nothing was counted).  load_pairs: a fresh
// table for `n` (key, count) pairs, counts of one key summed up to 255 -- the counter must hold no table (after split).
// Both synchronise `s`.  set_merged / merged: the mark a merged counter carries until it is reset (world 0: not merged).
int tab_split_by_owner(brx_counter *c, int world, hipStream_t s, uint64_t **d_keys, uint8_t **d_cnts, uint64_t *per_owner);
int tab_load_pairs(brx_counter *c, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, hipStream_t s);
// Key files (brx_keyfile.hip).  merge_pairs: load_pairs for a counter that may hold k-mers already -- the table is regrown for
// the k-mers known plus n, counts add up to 255; synchronises `s`.  floor: f > 1 after a count file that kept only counts
// >= f was loaded (finish below f - 1 and add_batch refuse until the counter is reset), 1 otherwise.  tab_info: what
// brx_counter_table_info reports.  set_alloc_unwritten (brx_set.hip): a set of this k with nothing written yet.
int tab_merge_pairs(brx_counter *c, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, hipStream_t s);
uint8_t tab_floor(const brx_counter *c);
void tab_set_floor(brx_counter *c, uint8_t floor);
int tab_info(brx_counter *c, uint64_t *info4, hipStream_t s);
int set_alloc_unwritten(int k, int device, brx_set **out);
// What set algebra (brx_setops.hip) shares with the key files (brx_keyfile.hip).  keys_scan_exclusive: d_data[0 .. n) in
// place, d_sums holds keys_scan_sums(n) + 1 entries and the last one receives the total.  keys_sort: brx_sort_keys_device.
// set_list_keys (brx_index.hip, on set_keys): the keys of a set, whatever holds it, into d_out, *sorted telling whether they are known to ascend (a key
// list marked so); the set is only read, a lazy bit vector stays lazy.  set_build_from_keys: makes a set_alloc_unwritten set the closed set of n sorted keys -- d_keys (exactly n entries,
// empty for n = 0) becomes its key list, a sparse set builds its chained index, the others write their bits and keep the
// list where index_wanted(k); `me` names the entry in messages.  keys_sort and set_build_from_keys return after `s` has been
// synchronised; set_list_keys leaves its copy queued on `s`.
uint64_t keys_scan_sums(uint64_t n);
int keys_scan_exclusive(unsigned long long *d_data, uint64_t n, unsigned long long *d_sums, hipStream_t s);
int keys_sort(uint64_t *d_keys, uint8_t *d_pay, uint64_t n, uint32_t key_bits, hipStream_t s);
int set_list_keys(const brx_set *set, hipStream_t s, DevBuf<uint64_t> &d_out, uint64_t *n_out, bool *sorted);
int set_build_from_keys(brx_set *set, DevBuf<uint64_t> &d_keys, uint64_t n, hipStream_t s, const char *me);
void tab_set_merged(brx_counter *c, int world, int rank);
bool tab_merged(const brx_counter *c, int *world, int *rank);
// Sliced counting (include/brx.h "sliced counting").  tab_set_slice: the counter must hold nothing (the caller holds its
// lock); the table it may still have is given back, so every slice sizes its own, and the peak starts again.  tab_slice:
// true for parts > 1.  tab_slice_stats synchronises `s`.
int tab_set_slice(brx_counter *c, uint32_t part, uint32_t parts);
bool tab_slice(const brx_counter *c, uint32_t *part, uint32_t *parts);
int tab_slice_stats(brx_counter *c, uint64_t *stats4, hipStream_t s);
int tab_reset(brx_counter *c, hipStream_t s);
int tab_spectrum(brx_counter *c, hipStream_t s, unsigned long long *d_hist);
// the rest of what brx_set.hip's counter entries call: the counting table (brx_counttable.hip) ...
int tab_begin(brx_counter *c);
void tab_free(brx_counter *c);
int tab_add_batch(brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                  hipStream_t s);
int tab_finish_into(brx_counter *c, uint32_t abundance, hipStream_t s, brx_set *dst);
// ... and the partitioned counter (brx_partbuild.hip)
bool part_supported(int k);
int part_begin(brx_counter *c);
void part_free(brx_counter *c);
int part_reset(brx_counter *c);
int part_add_batch(brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                   uint64_t total_bases, hipStream_t s);
int part_finish_into(brx_counter *c, uint32_t abundance, hipStream_t s, brx_set *dst);
int part_spectrum(brx_counter *c, hipStream_t s, unsigned long long *d_hist);
int part_l1_view(brx_counter *c, void **d_keys, void **d_l1off, uint32_t *n_buckets, uint64_t *n_keys);
int part_add_partitioned(brx_counter *c, const uint32_t *d_keys, const uint64_t *d_l1off, uint64_t n_keys);
// exclusive scan of n u32 lengths into n + 1 u64 offsets, the total also into *d_total (brx_scan.hip); d_tmp holds
// scan_tmp_bytes(n) bytes
uint64_t scan_tmp_bytes(uint32_t n);
int exclusive_scan_lens(const uint32_t *d_lens, uint32_t n, uint64_t *d_tmp, uint64_t *d_out_offsets,
                        unsigned long long *d_total, hipStream_t s);
// a host batch into the chain's staging buffers, offsets made relative to the first read (brx_set.hip)
int upload_batch(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, DevBuf<uint8_t> &d_bases, DevBuf<uint64_t> &d_off,
                 uint64_t *total, hipStream_t stream);
// count view of a BRX_COUNT_SORTED counter (brx_partbuild.hip); the callers hold the counter's lock.  part_lookup_view:
// false = no valid view; true with *keys == nullptr = nothing was counted.  part_lookup_shape: the buckets the offsets
// delimit and the positions behind them (brx_keyfile.hip walks the whole view to save it)
int part_lookup_prepare(brx_counter *c, hipStream_t s);
void part_lookup_drop(brx_counter *c);
bool part_lookup_ready(const brx_counter *c);
bool part_lookup_view(const brx_counter *c, const uint16_t **keys, const uint8_t **counts, const uint64_t **off);
bool part_lookup_shape(const brx_counter *c, uint64_t *n_buckets, uint64_t *n_positions);
// k-mer abundance of reads (brx_abundance.hip); the callers (brx_api.hip) hold the counter's lock.  abund_batch enqueues on
// `s` and returns after its kernels have completed
int abund_batch(const brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s);
int abund_get_counts(const brx_counter *c, const uint64_t *d_kmers, uint32_t n, uint8_t *d_out, hipStream_t s);
// what every batch entry does with a batch that has no k-mers to look up, before it asks for a view: *done = true when
// that was all -- no reads or no output asked for: nothing; reads without bases: histograms and statistics zeroed on `s`,
// which is synchronised
int abund_empty_batch(uint32_t n_reads, uint64_t total_bases, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats,
                      hipStream_t s, bool *done);
// sets the error of a partitioned counter that has no count view, returns BRX_ERR_UNSUPPORTED
int abund_refuse_partitioned(const char *what, int k);
// trusted stretches (brx_trust.hip): adds the five columns of n_reads statistics rows to d_tot5[0 .. 5), enqueued on `s`
int trust_totals_add(const brx_trust_stats_t *d_stats, uint32_t n_reads, unsigned long long *d_tot5, hipStream_t s);
}

// A count list (include/brx.h "count lists"): keys and counts are immutable once handed out, so they need no lock and no
// stream of their own.  The lookup directory (brx_listlookup.hip) is the one thing that comes and goes: prepare and drop
// hold lk_mu exclusively, the lookups hold it shared for as long as their kernels run, every other entry ignores it.
struct brx_counts {
    int k = 0;
    int device = 0;
    uint8_t floor = 1;            // every count is at least this; k-mers seen fewer times are unknown
    uint64_t n = 0;               // entries
    brx::DevBuf<uint64_t> d_keys; // strictly ascending; both empty when n == 0
    brx::DevBuf<uint8_t> d_cnts;
    mutable std::shared_mutex lk_mu;
    int lk_log2 = -1;             // log2 of the directory's buckets; -1: no directory, lookups refuse
    brx::DevBuf<uint64_t> d_dir;  // 2^lk_log2 + 1 offsets: d_dir[b] = number of keys < (b << (2k-1 - lk_log2))
    uint64_t lk_fullest = 0;      // keys in the fullest bucket
};

namespace brx {
// what the host-path entries of lists and set algebra share (brx_setops.hip, brx_listlookup.hip): the null check, and a
// stream of the call's own that is synchronised and destroyed when the call returns
inline int list_ok(const char *me, const brx_counts *l)
{
    if (!l) {
        set_error("%s: null count list", me);
        return BRX_ERR_ARG;
    }
    return BRX_OK;
}
struct OwnStream {
    hipStream_t s = nullptr;
    ~OwnStream()
    {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
};
// What a lookup reads of a prepared list (the caller holds lk_mu shared), and the two lookups over it (brx_abundance.hip):
// abund_batch / abund_get_counts with the list in the counter's place.
struct ListView {
    int k;
    const uint64_t *keys;
    const uint8_t *cnts;
    const uint64_t *dir;
    uint32_t shift; // bucket of key x = x >> shift
    uint64_t n;
};
int abund_batch_list(const ListView &l, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                     uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s);
int abund_get_counts_list(const ListView &l, const uint64_t *d_kmers, uint32_t n, uint8_t *d_out, hipStream_t s);
// The merge of two count lists into arrays sized from pass 1 (brx_setops.hip; timer "count_merge"): d_kout and, with
// want_counts, d_cout receive exactly *n_out entries (both reset when there are none); *both (may be null) = |A n B|.
// min_count is 1 .. 256 (256 keeps nothing: count > 255).  An empty B with BRX_COUNTOP_ADD is the compaction `count >=
// min_count`.  BRX_ERR_ARG for lists that do not ascend strictly or hold a 0 count.  Returns after `s` has been synchronised.
int counts_merge(const char *me, const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                 uint64_t nb, int op, uint32_t min_count, bool want_counts, hipStream_t s, DevBuf<uint64_t> &d_kout,
                 DevBuf<uint8_t> &d_cout, uint64_t *n_out, uint64_t *both);
}

struct brx_chain {
    const brx_set *set = nullptr;
    int device = 0;
    std::vector<brx_method_t> methods;
    bool two_side = false;   // second_pass == BRX_PASS_NONE
    int second_pass = BRX_PASS_REVERSE; // BRX_PASS_*
    hipStream_t stream = nullptr; // owned
    // workspace (grown on demand)
    brx::DevBuf<uint8_t> d_stage[2];
    brx::DevBuf<uint32_t> d_lens[2];
    brx::DevBuf<uint64_t> d_scan_tmp;
    brx::DevBuf<uint64_t> d_path;     // graph-walk visited lists (Graph / GapSize)
    brx::DevBuf<uint32_t> d_rev_list; // reads the lean reverse pass handed back (rev_scan_kernel)
    brx::DevBuf<uint32_t> d_rev_flag; // ... one word per read: entered into that list already
    brx::DevBuf<uint8_t> d_rev_trig;  // triggers the lean reverse pass left to the verify pass (TrigRec)
    brx::DevBuf<uint64_t> d_ctrl;     // device control block (work counter, overflow, stats)
    uint64_t *h_ctrl = nullptr;       // pinned mirror
    // host-entry staging
    brx::DevBuf<uint8_t> d_in, d_out;
    brx::DevBuf<uint64_t> d_off, d_out_off;
    uint64_t last_stats[8] = {};
    // workspace sizes that a batch of this chain has needed so far: the next batch starts from them, so that one
    // long walk or one read that grows a lot costs its own batch a second run, not every batch after it
    uint32_t slack_seen = 1, maxpath_seen = 4096;
    // second chain (same set, methods and direction rule, its own workspace) that redoes the few reads of a batch
    // whose graph walks outgrew the visited list; created on first need
    brx_chain *sub = nullptr;
    bool is_sub = false;
    void *lane_ws = nullptr; // workspace of the lane-per-chunk pass (brx_onelane.hip)
    uint8_t *h_in = nullptr; // page-locked bounce block for batches handed over in pageable memory
    uint64_t h_in_cap = 0;
    void *async_job = nullptr; // a batch in flight (brx_chain_correct_batch_async), owned by the chain
    std::mutex mu;
};

namespace brx {
struct CorrectTuning; // the correction switches as one batch sees them (brx_plan.hpp)
// the chain's entries under a tuning record the caller has read (brx_pipeline.hip reads one per run, on the calling
// thread, and hands it to its workers): what brx_chain_new_pass and brx_chain_correct_batch_device do (brx_correct.hip)
int chain_new(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, int second_pass, const CorrectTuning &tuning,
              brx_chain_t **out);
int chain_correct_batch_device(brx_chain_t *ch, const CorrectTuning &tuning, const uint8_t *d_bases, const uint64_t *d_offsets,
                               uint32_t n_reads, uint64_t total_bases, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                               uint64_t *out_total, void *stream);
}
