// Probe index: an HBM-locality layout of the solid set, used by the correction kernels.
//
// The reference's KmerSet::get (src/set/pcon.rs:189-191) is one bit of a 2^(2k-1)-bit vector, and the
// canonical hashes of the k-mers a read walks through are unrelated: every get is its own 64-byte
// memory transaction, and MI355X sustains ~55 G such transactions per second whatever the kernel does
// (tools/line_probe_bench.hip).  The same tool shows that lanes of a wave reading the SAME line cost one
// transaction.  So the solid k-mers are also stored in 64-byte lines addressed by the k-mer's
// strand-symmetric MINIMIZER (smallest hashed canonical m-mer inside the k-mer): consecutive k-mers of a
// read share their minimizer for (k-m+2)/2 positions on average and the lanes that probe them share the
// line.  The index is exact: a line lists full keys; a line that could not take all its keys is flagged
// and a probe it cannot answer is re-issued against the bitset, which stays the source of truth -- or, for
// sparse sets (k >= 21, no bit vector), against the next line, where the build chained the key to.
//
// Line layout (8 x u64): [0..6] key+1 of up to 7 k-mers (0 = empty; key = canonical >> 1),
// [7] header: low 32 bits = number of insert attempts, bit 63 = overflowed.
#pragma once
#include "brx_kmer.hpp"

struct brx_set;

namespace brx {

constexpr int IDX_SLOTS = 7;
constexpr uint64_t IDX_OVERFLOW = 1ull << 63;
// bits 32..62 of a line's header: a 31-bit signature of the keys that did not fit THEIR HOME line (the line their
// minimizer addresses).  A probe that finds its home line flagged but its own signature bit clear is a definite
// "absent" -- without it every probe of a flagged line, present or not, costs its group a second round.
// (32-bit multiply of the key's low word, top 5 bits, 31 folded onto 30: five instructions in the probe instead of a
// 64-bit multiply and a modulo)
__host__ __device__ inline uint32_t idx_sig_index(uint64_t key)
{
    const uint32_t t = ((uint32_t)key * 0x9E3779B1u) >> 27;
    return t > 30u ? 30u : t;
}
__host__ __device__ inline uint64_t idx_sig_bit(uint64_t key) { return 1ull << (32u + idx_sig_index(key)); }
constexpr int IDX_MAX_M = 16; // a canonical m-mer must fit 32 bits (32-bit window arithmetic); 16 needs no masking
constexpr int IDX_AUTO_MAX_M = 15; // what index_auto_m picks by itself (odd lengths; BRX_INDEX_M / the ABI may ask for 16)

struct IdxView {
    const uint64_t *lines; // nullptr: no index, probe the bitset
    uint32_t line_shift;   // 32 - log2(number of lines)
    uint32_t m;            // minimizer length (odd, <= 15)
    uint32_t w;            // k - m + 1 windows
    // one bit per line: set = the line holds at least one key.  4 MiB for 2^25 lines, i.e. L2-resident: a probe whose
    // home line is empty is "absent" without fetching the line from HBM (79 % of the lines of the bench's set are empty,
    // and the reverse pass of run_correction probes almost only absent k-mers).  nullptr: not kept for this index.
    const uint32_t *line_bits = nullptr;
};

// How a kernel reaches a set (brx_index.hip): the bit vector -- nullptr for a sparse set and for a lazy one, which stays
// lazy -- and the index, lines == nullptr where the set has none or, unless any_index, where k is outside the indexed
// range and the bit vector answers.  line_bits false: the occupancy bits are not handed out (BRX_LINE_BITS=0).
struct SetView {
    const uint32_t *bits;
    IdxView idx;
};
SetView set_view(const brx_set *set, bool line_bits, bool any_index = false);

// What one launch enumerates (for_each_key): a key list (`n` clamped on the host to what the list holds), the entries of a
// table's lines (8 per line, the header among them) or the words of a bit vector -- the first pointer that is set.
struct KeySource {
    const uint64_t *keys = nullptr;
    uint64_t n = 0;
    const uint64_t *lines = nullptr;
    uint64_t n_entries = 0;
    const uint32_t *bits = nullptr;
    uint64_t nwords = 0;
};
inline KeySource list_source(const uint64_t *keys, uint64_t n) { KeySource s; s.keys = keys; s.n = n; return s; }
inline KeySource table_source(const uint64_t *lines, uint64_t n_lines) { KeySource s; s.lines = lines; s.n_entries = n_lines * 8ull; return s; }
inline KeySource bits_source(const uint32_t *bits, uint64_t nwords) { KeySource s; s.bits = bits; s.nwords = nwords; return s; }

#if defined(__HIPCC__)

// entry i of a table's lines as a slot: the key + 1, 0 for an empty slot and for the line's header (entry 7)
__device__ __forceinline__ uint64_t table_slot_key(const uint64_t *__restrict__ lines, uint64_t i)
{
    return (i & 7ull) == 7ull ? 0ull : lines[i];
}

// f(key) for every key of the source (key = canonical >> 1), each once, in a grid-stride loop; the kind is uniform per launch
template <class F>
__device__ __forceinline__ void for_each_key(const KeySource &src, F f)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (src.keys)
        for (uint64_t i = first; i < src.n; i += stride)
            f(src.keys[i]);
    else if (src.lines)
        for (uint64_t i = first; i < src.n_entries; i += stride) {
            if (const uint64_t v = table_slot_key(src.lines, i))
                f(v - 1ull);
        }
    else
        for (uint64_t w = first; w < src.nwords; w += stride)
            for (uint32_t x = src.bits[w]; x; x &= x - 1u)
                f(w * 32ull + (uint64_t)(__ffs(x) - 1));
}

// hash of the minimizer of a k-mer: min over its W m-mers of (min(m-mer, revcomp(m-mer)) * odd) mod 2^32,
// an injective order of the canonical m-mers, so equal hashes mean equal minimizers.
// The m-mer at bit offset 2j of fwd is the revcomp of the m-mer at bit offset 2(W-1-j) of rc, so the
// value is the same for a k-mer and its reverse complement.
template <int W>
__device__ __forceinline__ uint32_t minimizer_hash_w(uint64_t fwd, uint64_t rc, uint32_t mm)
{
    const uint32_t flo = (uint32_t)fwd, fhi = (uint32_t)(fwd >> 32), rlo = (uint32_t)rc, rhi = (uint32_t)(rc >> 32);
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < W; j++) {
        const uint32_t f = __builtin_amdgcn_alignbit(fhi, flo, 2 * j) & mm;
        const uint32_t r = __builtin_amdgcn_alignbit(rhi, rlo, 2 * (W - 1 - j)) & mm;
        const uint32_t c = f < r ? f : r;
        const uint32_t h = c * 0x9E3779B1u; // (a full-rate xor+rotate scramble measured no faster: the kernel waits on memory)
        best = h < best ? h : best;
    }
    return best;
}

__device__ __forceinline__ uint32_t minimizer_of(uint64_t fwd, uint64_t rc, uint32_t m, uint32_t w);
// the same, also giving the minimum over all windows but the OLDEST one (the m-mer at the front of the k-mer): the k-mer
// that follows in a read shares exactly those W - 1 windows, so its minimizer is min(excl_oldest, hash of its one new
// m-mer) -- brx_onelane.hip asks about two consecutive positions per round that way
template <int W>
__device__ __forceinline__ uint32_t minimizer_hash_w2(uint64_t fwd, uint64_t rc, uint32_t mm, uint32_t &excl_oldest)
{
    const uint32_t flo = (uint32_t)fwd, fhi = (uint32_t)(fwd >> 32), rlo = (uint32_t)rc, rhi = (uint32_t)(rc >> 32);
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < W - 1; j++) {
        const uint32_t f = __builtin_amdgcn_alignbit(fhi, flo, 2 * j) & mm;
        const uint32_t r = __builtin_amdgcn_alignbit(rhi, rlo, 2 * (W - 1 - j)) & mm;
        const uint32_t c = f < r ? f : r;
        const uint32_t h = c * 0x9E3779B1u;
        best = h < best ? h : best;
    }
    excl_oldest = best;
    const uint32_t f = __builtin_amdgcn_alignbit(fhi, flo, 2 * (W - 1)) & mm;
    const uint32_t r = rlo & mm;
    const uint32_t c = f < r ? f : r;
    const uint32_t h = c * 0x9E3779B1u;
    return h < best ? h : best;
}

// false: more than 16 windows (no two-position rounds there)
__device__ __forceinline__ bool minimizer_pair(uint64_t fwd, uint64_t rc, uint32_t m, uint32_t w, uint32_t &best, uint32_t &excl_oldest)
{
    const uint32_t mm = m >= 16u ? 0xffffffffu : (1u << (2u * m)) - 1u;
    switch (w) { // wave-uniform
    case 2: best = minimizer_hash_w2<2>(fwd, rc, mm, excl_oldest); return true;
    case 3: best = minimizer_hash_w2<3>(fwd, rc, mm, excl_oldest); return true;
    case 4: best = minimizer_hash_w2<4>(fwd, rc, mm, excl_oldest); return true;
    case 5: best = minimizer_hash_w2<5>(fwd, rc, mm, excl_oldest); return true;
    case 6: best = minimizer_hash_w2<6>(fwd, rc, mm, excl_oldest); return true;
    case 7: best = minimizer_hash_w2<7>(fwd, rc, mm, excl_oldest); return true;
    case 8: best = minimizer_hash_w2<8>(fwd, rc, mm, excl_oldest); return true;
    case 9: best = minimizer_hash_w2<9>(fwd, rc, mm, excl_oldest); return true;
    case 10: best = minimizer_hash_w2<10>(fwd, rc, mm, excl_oldest); return true;
    case 11: best = minimizer_hash_w2<11>(fwd, rc, mm, excl_oldest); return true;
    case 12: best = minimizer_hash_w2<12>(fwd, rc, mm, excl_oldest); return true;
    case 13: best = minimizer_hash_w2<13>(fwd, rc, mm, excl_oldest); return true;
    case 14: best = minimizer_hash_w2<14>(fwd, rc, mm, excl_oldest); return true;
    case 15: best = minimizer_hash_w2<15>(fwd, rc, mm, excl_oldest); return true;
    case 16: best = minimizer_hash_w2<16>(fwd, rc, mm, excl_oldest); return true;
    default:
        best = minimizer_of(fwd, rc, m, w);
        excl_oldest = 0;
        return false;
    }
}

__device__ __forceinline__ uint32_t minimizer_of(uint64_t fwd, uint64_t rc, uint32_t m, uint32_t w)
{
    const uint32_t mm = m >= 16u ? 0xffffffffu : (1u << (2u * m)) - 1u;
    switch (w) { // wave-uniform
    case 2: return minimizer_hash_w<2>(fwd, rc, mm);
    case 3: return minimizer_hash_w<3>(fwd, rc, mm);
    case 4: return minimizer_hash_w<4>(fwd, rc, mm);
    case 5: return minimizer_hash_w<5>(fwd, rc, mm);
    case 6: return minimizer_hash_w<6>(fwd, rc, mm);
    case 7: return minimizer_hash_w<7>(fwd, rc, mm);
    case 8: return minimizer_hash_w<8>(fwd, rc, mm);
    case 9: return minimizer_hash_w<9>(fwd, rc, mm);
    case 10: return minimizer_hash_w<10>(fwd, rc, mm);
    case 11: return minimizer_hash_w<11>(fwd, rc, mm);
    case 12: return minimizer_hash_w<12>(fwd, rc, mm);
    case 13: return minimizer_hash_w<13>(fwd, rc, mm);
    case 14: return minimizer_hash_w<14>(fwd, rc, mm);
    case 15: return minimizer_hash_w<15>(fwd, rc, mm);
    case 16: return minimizer_hash_w<16>(fwd, rc, mm);
    default: { // more than 16 windows (k >= 31 with m = 15): 64-bit shifts
        uint32_t best = 0xffffffffu;
        for (uint32_t j = 0; j < w; j++) {
            const uint32_t f = (uint32_t)(fwd >> (2u * j)) & mm;
            const uint32_t r = (uint32_t)(rc >> (2u * (w - 1u - j))) & mm;
            const uint32_t c = f < r ? f : r;
            const uint32_t h = c * 0x9E3779B1u;
            best = h < best ? h : best;
        }
        return best;
    }
    }
}

// the minimum of W hashes crowds the low end of the range: multiply once more before taking the top bits
__device__ __forceinline__ uint32_t index_line_of(uint32_t mh, uint32_t line_shift)
{
    return (mh * 0x85EBCA6Bu) >> line_shift;
}

// 1 = present, 0 = absent, 2 = the line overflowed and does not hold the key: ask the bit vector, or -- sparse sets,
// whose keys chain into the following lines -- probe again with hop + 1
// the key of a forward k-mer (canonical >> 1, + 1) and its home line
__device__ __forceinline__ uint32_t index_locate(const IdxView &v, uint64_t fwd, int k, uint64_t &key)
{
    const uint64_t rc = revcomp(fwd, k);
    key = (((popc64(fwd) & 1) ? rc : fwd) >> 1) + 1ull;
    return index_line_of(minimizer_of(fwd, rc, v.m, v.w), v.line_shift);
}

__device__ __forceinline__ int index_probe_at(const IdxView &v, uint64_t key, uint32_t home, uint32_t hop)
{
    const uint32_t line = (home + hop) & (0xffffffffu >> v.line_shift);
    const ulonglong2 *L = reinterpret_cast<const ulonglong2 *>(v.lines + (uint64_t)line * 8ull);
    const ulonglong2 q0 = L[0], q1 = L[1], q2 = L[2], q3 = L[3];
    // `|`, not `||`: with short-circuit evaluation the compiler loads slot 0 first and fetches the rest of
    // the line only for the lanes that did not match it -- a second, dependent memory round trip
    const bool found = (q0.x == key) | (q0.y == key) | (q1.x == key) | (q1.y == key) | (q2.x == key) | (q2.y == key) | (q3.x == key);
    // home line (hop 0): go on only if one of the keys it turned away had this key's signature; further down a
    // chain only the flag can tell
    const uint32_t hdr_hi = (uint32_t)(q3.y >> 32); // bit 31 = overflowed, bits 0..30 = signature of the keys turned away
    const bool more = (hdr_hi >> 31) && (hop != 0u || ((hdr_hi >> idx_sig_index(key)) & 1u));
    return found ? 1 : (more ? 2 : 0);
}

__device__ __forceinline__ int index_probe(const IdxView &v, uint64_t fwd, int k, uint32_t hop = 0)
{
    uint64_t key;
    const uint32_t home = index_locate(v, fwd, k, key);
    return index_probe_at(v, key, home, hop);
}

// index_probe through the line-occupancy bits: an empty home line answers "absent" from a 4-byte load that hits L2
__device__ __forceinline__ int index_probe_filtered(const IdxView &v, uint64_t fwd, int k)
{
    uint64_t key;
    const uint32_t home = index_locate(v, fwd, k, key);
    if (!((v.line_bits[home >> 5] >> (home & 31u)) & 1u))
        return 0;
    return index_probe_at(v, key, home, 0u);
}
// one bit of the bit vector
__device__ __forceinline__ bool probe(const uint32_t *__restrict__ bits, uint64_t fwd, int k)
{
    const uint64_t h = khash(fwd, k);
    return (bits[h >> 5] >> (h & 31u)) & 1u;
}

// KmerSet::get of one forward k-mer (src/set/pcon.rs:189-191), whatever holds the set: THE definition, every kernel
// that asks goes through it.  IDX = false: the bit vector.  IDX = true: the probe index with "cannot say" settled on
// the spot -- the lane asks the bit vector when there is one, else (sets without one chain their overflowed keys into
// the following lines) the next lines of the chain, never more of them than the index has.  One probe in a thousand
// at configs[1]'s occupancy; the other lanes of the wave wait for it.  TELL: *home_answer = what the home line said
// (0, 1, or 2 = cannot say).
// The occupancy bits: an empty home line answers "absent" from its bit, and most k-mers with an error point at one.  When
// the bits are consulted -- given that the index keeps them and the host handed them out -- is the caller's LB:
//   LINE_BITS_IN_L2  a wave asks about 64 neighbouring positions per step (lane_mask_kernel; cover_kernel's cover_get): while the
//                    bits live in the L2, i.e. at most 2^26 lines (4 MiB at 2^25).  Past that every lookup is a request
//                    of its own on top of the line's (BASELINE configs[4]'s share, 2^28 lines: lane_mask_kernel 40.1 ms
//                    with the bits, 35.1 without);
//   LINE_BITS_KEPT   the group kernels' scans and walks (brx_group.hip, brx_one.hip, brx_revscan.hip): always;
//   LINE_BITS_NEVER  single probes (lane_sync_kernel, succ_build_kernel, index_get_kernel).
// (LB and TELL are template parameters so that each caller compiles to the code it had when it wrote this out itself.)
enum LineBitsUse { LINE_BITS_NEVER, LINE_BITS_KEPT, LINE_BITS_IN_L2 };
template <bool IDX, LineBitsUse LB, bool TELL = false>
__device__ __forceinline__ bool set_get(const IdxView &v, const uint32_t *__restrict__ bits, uint64_t fwd, int k, int *home_answer = nullptr)
{
    if (!IDX)
        return probe(bits, fwd, k);
    if (TELL)
        *home_answer = 0;
    uint64_t key;
    const uint32_t home = index_locate(v, fwd, k, key);
    if (LB != LINE_BITS_NEVER && v.line_bits && (LB == LINE_BITS_KEPT || v.line_shift >= 6u) &&
        !((v.line_bits[home >> 5] >> (home & 31u)) & 1u))
        return false;
    int a = index_probe_at(v, key, home, 0u);
    if (TELL)
        *home_answer = a;
    if (a == 2) {
        if (bits) {
            const uint64_t h = khash(fwd, k);
            return (bits[h >> 5] >> (h & 31u)) & 1u;
        }
        const uint32_t last = 0xffffffffu >> v.line_shift;
        for (uint32_t hop = 1; a == 2 && hop <= last; hop++)
            a = index_probe_at(v, key, home, hop);
    }
    return a == 1;
}

// find-or-insert of one k-mer into a chained table (sparse sets filled k-mer by k-mer, `br large-kmer`): true if the
// key was not there.  Threads race for the first empty slot of a line with a CAS; slots never empty again, so
// all threads see the same first empty slot and a key cannot land twice.
__device__ __forceinline__ bool table_find_or_insert(uint64_t *lines, uint32_t line_shift, uint32_t m, uint32_t w, int k, uint64_t fwd)
{
    const uint64_t rc = revcomp(fwd, k);
    const unsigned long long key = (((popc64(fwd) & 1) ? rc : fwd) >> 1) + 1ull;
    const uint32_t line_mask = 0xffffffffu >> line_shift;
    uint32_t line = index_line_of(minimizer_of(fwd, rc, m, w), line_shift);
    bool first = true; // still at the key's home line
    for (;;) {
        unsigned long long *L = reinterpret_cast<unsigned long long *>(lines) + (uint64_t)line * 8ull;
        for (int j = 0; j < IDX_SLOTS; j++) {
            unsigned long long v = __hip_atomic_load(L + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == 0ull)
                v = atomicCAS(L + j, 0ull, key);
            if (v == 0ull)
                return true;
            if (v == key)
                return false;
        }
        {
            const unsigned long long want = (unsigned long long)IDX_OVERFLOW | (first ? (unsigned long long)idx_sig_bit(key) : 0ull);
            if ((__hip_atomic_load(L + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & want) != want)
                atomicOr(L + 7, want);
        }
        first = false;
        line = (line + 1u) & line_mask; // the table is kept at most half full: this ends
    }
}

// Counting table (BRX_COUNT_TABLE, brx_counttable.hip): the same chained table with one u32 counter per slot in an
// array of its own, counts[line * 8 + slot] (entry 7 of a line is never used), so that the lines keep their format.
// table_find_or_insert's walk, giving the index of the key's slot (`fresh`: this call put the key there).  The key
// goes in with the one CAS, so no slot is ever claimed but unfilled and nobody waits for anybody.
__device__ __forceinline__ uint64_t table_find_or_claim(uint64_t *lines, uint32_t line_shift, uint32_t m, uint32_t w, int k, uint64_t fwd,
                                                        bool &fresh)
{
    const uint64_t rc = revcomp(fwd, k);
    const unsigned long long key = (((popc64(fwd) & 1) ? rc : fwd) >> 1) + 1ull;
    const uint32_t line_mask = 0xffffffffu >> line_shift;
    uint32_t line = index_line_of(minimizer_of(fwd, rc, m, w), line_shift);
    bool first = true;
    for (;;) {
        unsigned long long *L = reinterpret_cast<unsigned long long *>(lines) + (uint64_t)line * 8ull;
        for (int j = 0; j < IDX_SLOTS; j++) {
            unsigned long long v = __hip_atomic_load(L + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            fresh = false;
            if (v == 0ull) {
                v = atomicCAS(L + j, 0ull, key);
                fresh = v == 0ull;
            }
            if (fresh || v == key)
                return (uint64_t)line * 8ull + (uint64_t)j;
        }
        {
            const unsigned long long want = (unsigned long long)IDX_OVERFLOW | (first ? (unsigned long long)idx_sig_bit(key) : 0ull);
            if ((__hip_atomic_load(L + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & want) != want)
                atomicOr(L + 7, want);
        }
        first = false;
        line = (line + 1u) & line_mask; // the host keeps the table at most about half full: this ends
    }
}

// Read-only twin of table_find_or_claim (brx_abundance.hip): the index of the slot that holds `key`, or TAB_NO_SLOT.  The
// walk of index_probe_at: the whole line in four 16-byte loads, the seven slots compared with `|`; a miss goes on to the
// next line only while the line is flagged, and at the home line only if one of the keys it turned away had this key's
// signature.  Never more lines than the table has, so a damaged table cannot keep a wave here for ever.  Plain loads:
// nothing counts while this runs (the counter's lock and the stream's order see to that).
constexpr uint64_t TAB_NO_SLOT = ~0ull;
__device__ __forceinline__ uint64_t table_lookup_slot(const uint64_t *__restrict__ lines, uint32_t line_shift, uint64_t key, uint32_t home)
{
    const uint32_t line_mask = 0xffffffffu >> line_shift;
    for (uint32_t hop = 0;; hop++) {
        const uint32_t line = (home + hop) & line_mask;
        const ulonglong2 *L = reinterpret_cast<const ulonglong2 *>(lines + (uint64_t)line * 8ull);
        const ulonglong2 q0 = L[0], q1 = L[1], q2 = L[2], q3 = L[3];
        const uint32_t hit = (uint32_t)(q0.x == key) | ((uint32_t)(q0.y == key) << 1) | ((uint32_t)(q1.x == key) << 2) |
                             ((uint32_t)(q1.y == key) << 3) | ((uint32_t)(q2.x == key) << 4) | ((uint32_t)(q2.y == key) << 5) |
                             ((uint32_t)(q3.x == key) << 6);
        if (hit)
            return (uint64_t)line * 8ull + (uint64_t)(__ffs((int)hit) - 1);
        const uint32_t hdr_hi = (uint32_t)(q3.y >> 32);
        const bool more = (hdr_hi >> 31) && (hop != 0u || ((hdr_hi >> idx_sig_index(key)) & 1u));
        if (!more || hop == line_mask)
            return TAB_NO_SLOT;
    }
}

constexpr uint32_t TAB_COUNT_MAX = 255u; // what a counter is read as at most (pcon's Counter<u8>)
// One more occurrence.  A counter that has reached 255 is left alone, so it stands for min(255, occurrences) however
// long the input: lanes that all saw 254 may each add their one, which leaves it above 255 by less than the number of
// threads in flight (far from 2^32, and every reader takes min(255, .)).  One atomic add on the slot's own word: no
// retry loop, nothing carried into a neighbour, and lanes of a wave that hit one slot are serialised by the memory system.
__device__ __forceinline__ void table_count_bump(uint32_t *counter, uint32_t by = 1u)
{
    if (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < TAB_COUNT_MAX)
        atomicAdd(counter, by);
}
__device__ __forceinline__ uint32_t table_count_read(uint32_t v) { return v < TAB_COUNT_MAX ? v : TAB_COUNT_MAX; }
#endif

} // namespace brx
