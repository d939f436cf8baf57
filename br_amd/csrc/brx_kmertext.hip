// K-mer text (include/brx.h "k-mer text"; br_amd/kmertext.py states the form in numpy): count lists to and from
// `KMER<TAB>COUNT` lines.  What a lane does with one entry or one line is brx_kmertext.hpp; here are the stream kernels
// around it and the host paths.
//
//   format   blocks of 256 entries.  text_measure_kernel: the bytes of each block's lines; an exclusive scan of them
//            (brx_keyfile.hip's); text_write_kernel: a lane writes its line into LDS at the place a block scan gives it, the
//            block's bytes lying in LDS as they will lie in memory modulo 16, and the block stores its contiguous range
//            once -- whole 16-byte chunks, and single bytes only in the chunk it shares with a neighbour at either end.
//   parse    nl_count_kernel: the '\n' of each 4096 bytes (16 per lane, one load where the text is aligned); a scan;
//            nl_scatter_kernel: line j starts behind the j-th '\n', line 0 at byte 0, and the bytes behind the last '\n'
//            are one more line.  line_count_kernel: the non-empty lines of each 256 lines; a scan; text_parse_kernel: a
//            lane parses its line and writes its pair where the scan puts it, so the pairs stand in line order; a
//            malformed line enters an atomic min over line indices, and text_cause_kernel, one lane, reads that line again
//            for cause and column.  No workgroup waits for another: what one step leaves is read by the next launch.
//   run-sum  (import) over the sorted pairs: head_count_kernel counts the keys that differ from the key before them, a
//            scan, runsum_kernel: a head lane walks its run -- across block borders, and no further than the 255 entries
//            after which a sum is saturated -- and writes its key with the sum.
// The host paths pass the text through the pieces of the key files (brx_keyio.hpp).
#include "brx_internal.hpp"
#include "brx_keyio.hpp"
#include "brx_kmertext.hpp"

#include <string.h>

using namespace brx;

namespace {

typedef unsigned long long u64;

constexpr uint32_t TB = 256;        // entries (lines) per block trip
constexpr uint32_t NL_CHUNK = 4096; // bytes per block trip of the newline kernels
constexpr uint32_t TEXT_LDS = TB * TEXT_MAX_LINE + 32; // the lines of a block, up to 15 bytes in front of them
constexpr u64 NONE = ~0ull;

uint32_t grid_for(uint64_t trips) { return read_grid(trips ? trips : 1, 256u * 16u); }
uint64_t blocks_of(uint64_t n, uint32_t per) { return (n + per - 1) / per; }

// ---- format ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_measure_kernel(const uint8_t *__restrict__ cnts, uint64_t n, uint64_t n_blocks, int k,
                                                           u64 *__restrict__ size)
{
    __shared__ u64 sh[4];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        const uint64_t i = b * TB + threadIdx.x;
        const u64 len = i < n ? text_line_len(k, cnts[i]) : 0u;
        u64 total;
        (void)block_excl_scan(len, sh, &total);
        if (threadIdx.x == 0)
            size[b] = total;
    }
}

// sizes[j] = bytes of the lines of entries [j * per, min(n, (j + 1) * per)): what the host needs to know of a slice
__global__ __launch_bounds__(256) void text_slice_sizes_kernel(const uint8_t *__restrict__ cnts, uint64_t n, uint64_t per, uint64_t n_slices,
                                                               int k, u64 *__restrict__ sizes)
{
    __shared__ u64 sh[4];
    for (uint64_t j = blockIdx.x; j < n_slices; j += gridDim.x) { // block-uniform
        const uint64_t lo = j * per, hi = n - lo < per ? n : lo + per;
        u64 sum = 0;
        for (uint64_t i = lo + threadIdx.x; i < hi; i += 256u)
            sum += text_line_len(k, cnts[i]);
        u64 total;
        (void)block_excl_scan(sum, sh, &total);
        if (threadIdx.x == 0)
            sizes[j] = total;
    }
}

// off: the scanned sizes.  Block b's bytes are out[off[b] .. off[b] + its total)
__global__ __launch_bounds__(256) void text_write_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ cnts, uint64_t n,
                                                         uint64_t n_blocks, int k, uint32_t lex, const u64 *__restrict__ off,
                                                         uint64_t out_bytes, uint8_t *__restrict__ out)
{
    __shared__ u64 sh[4];
    __shared__ uint4 buf4[TEXT_LDS / 16];
    uint8_t *buf = reinterpret_cast<uint8_t *>(buf4);
    const uint32_t tid = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        const uint64_t i = b * TB + tid;
        const uint32_t cnt = i < n ? cnts[i] : 0u;
        const u64 len = i < n ? text_line_len(k, cnt) : 0u;
        u64 total;
        const u64 before = block_excl_scan(len, sh, &total);
        const uint64_t o = off[b];
        const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(out + o) & 15u); // where the block's bytes start inside their 16
        if (i < n)
            (void)text_format_line(k, keys[i], cnt, lex != 0u, buf + a + (uint32_t)before); // (a + before + len <= 15 + 256 * 36)
        __syncthreads();
        if (o + total <= out_bytes) { // (always: the sizes were measured over the same counts)
            uint8_t *g = out + o - a; // 16-byte aligned; bytes [a, end) of it are this block's
            const uint32_t end = a + (uint32_t)total;
            const uint32_t c_lo = a ? 1u : 0u, c_hi = end / 16u; // the whole chunks
            for (uint32_t c = c_lo + tid; c < c_hi; c += 256u)
                reinterpret_cast<uint4 *>(g)[c] = buf4[c];
            if (tid < 16u) {
                if (a && tid >= a && tid < end) // the chunk shared with the block before
                    g[tid] = buf[tid];
                const uint32_t t = (c_hi > c_lo ? c_hi : c_lo) * 16u + tid; // ... and with the block behind
                if (t < end)
                    g[t] = buf[t];
            }
        }
        __syncthreads(); // (buf is written again in the next trip)
    }
}

// measure + scan of n entries on `s`: d_size (blocks_of(n, TB) entries) scanned, the total in d_sums[keys_scan_sums(blocks)]
int format_measure(int k, const uint8_t *d_cnts, uint64_t n, u64 *d_size, u64 *d_sums, hipStream_t s)
{
    const uint64_t nb = blocks_of(n, TB);
    text_measure_kernel<<<grid_for(nb), 256, 0, s>>>(d_cnts, n, nb, k, d_size);
    BRX_HIP(hipGetLastError());
    return keys_scan_exclusive(d_size, nb, d_sums, s);
}

int format_write(int k, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, int strand, const u64 *d_size, uint64_t out_bytes,
                 uint8_t *d_text, hipStream_t s)
{
    const uint64_t nb = blocks_of(n, TB);
    text_write_kernel<<<grid_for(nb), 256, 0, s>>>(d_keys, d_cnts, n, nb, k, strand == BRX_TEXT_LEX ? 1u : 0u, d_size, out_bytes, d_text);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// ---- parse ----------------------------------------------------------------------------------------------------------------
// bit j: text[at + j] is '\n' (at % 16 == 0; bytes past the end are none)
__device__ __forceinline__ uint32_t nl_mask16(const uint8_t *__restrict__ text, uint64_t at, uint64_t bytes, bool aligned)
{
    uint32_t m = 0;
    if (at >= bytes)
        return 0u;
    if (aligned && at + 16u <= bytes) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t q = 0; q < 4u; q++)
            for (uint32_t r = 0; r < 4u; r++)
                if (((w[q] >> (8u * r)) & 0xFFu) == 10u)
                    m |= 1u << (4u * q + r);
    } else {
        for (uint32_t j = 0; j < 16u && at + j < bytes; j++)
            if (text[at + j] == 10u)
                m |= 1u << j;
    }
    return m;
}

__global__ __launch_bounds__(256) void nl_count_kernel(const uint8_t *__restrict__ text, uint64_t bytes, uint64_t n_chunks, uint32_t aligned,
                                                       u64 *__restrict__ cnt)
{
    __shared__ u64 sh[4];
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) { // block-uniform
        const uint32_t m = nl_mask16(text, c * NL_CHUNK + 16ull * threadIdx.x, bytes, aligned != 0u);
        u64 total;
        (void)block_excl_scan((u64)__popc(m), sh, &total);
        if (threadIdx.x == 0)
            cnt[c] = total;
    }
}

// cnt: scanned.  starts[0] = 0, starts[j] = the byte behind the j-th '\n'; n_starts = their number + 1
__global__ __launch_bounds__(256) void nl_scatter_kernel(const uint8_t *__restrict__ text, uint64_t bytes, uint64_t n_chunks, uint32_t aligned,
                                                         const u64 *__restrict__ cnt, u64 *__restrict__ starts, uint64_t n_starts)
{
    __shared__ u64 sh[4];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        starts[0] = 0;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) { // block-uniform
        const uint64_t at = c * NL_CHUNK + 16ull * threadIdx.x;
        uint32_t m = nl_mask16(text, at, bytes, aligned != 0u);
        u64 total;
        uint64_t pos = cnt[c] + block_excl_scan((u64)__popc(m), sh, &total) + 1ull;
        while (m) {
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            if (pos < n_starts) // (always: the counts were taken over the same text)
                starts[pos] = at + j + 1ull;
            pos++;
        }
    }
}

// line j of the text: its first byte and its length without '\n' and without one '\r' before it
__device__ __forceinline__ uint64_t line_of(const uint8_t *__restrict__ text, uint64_t bytes, const u64 *__restrict__ starts, uint64_t n_lines,
                                            uint64_t j, const uint8_t **p)
{
    const uint64_t lo = starts[j], hi = j + 1 < n_lines ? starts[j + 1] - 1ull : bytes;
    *p = text + lo;
    return hi > lo && hi <= bytes ? text_trim(text + lo, hi - lo) : 0ull;
}

__global__ __launch_bounds__(256) void line_count_kernel(const uint8_t *__restrict__ text, uint64_t bytes, const u64 *__restrict__ starts,
                                                         uint64_t n_lines, uint64_t n_blocks, u64 *__restrict__ cnt)
{
    __shared__ u64 sh[4];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        const uint64_t j = b * TB + threadIdx.x;
        const uint8_t *p;
        const u64 some = j < n_lines && line_of(text, bytes, starts, n_lines, j, &p) ? 1u : 0u;
        u64 total;
        (void)block_excl_scan(some, sh, &total);
        if (threadIdx.x == 0)
            cnt[b] = total;
    }
}

// cnt: scanned.  ctl[0]: the first malformed line (NONE before the launch)
__global__ __launch_bounds__(256) void text_parse_kernel(const uint8_t *__restrict__ text, uint64_t bytes, const u64 *__restrict__ starts,
                                                         uint64_t n_lines, uint64_t n_blocks, int k, const u64 *__restrict__ cnt,
                                                         uint64_t *__restrict__ keys, uint8_t *__restrict__ cnts, uint64_t cap,
                                                         u64 *__restrict__ ctl)
{
    __shared__ u64 sh[4];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        const uint64_t j = b * TB + threadIdx.x;
        const uint8_t *p = text;
        const uint64_t len = j < n_lines ? line_of(text, bytes, starts, n_lines, j, &p) : 0ull;
        u64 total;
        const uint64_t pos = cnt[b] + block_excl_scan(len ? 1u : 0u, sh, &total);
        if (len) {
            uint64_t key = 0, col = 0;
            uint32_t count = 0;
            if (text_parse_line(p, len, k, &key, &count, &col) != TEXT_OK)
                atomicMin(ctl, (u64)j);
            else if (pos < cap) {
                keys[pos] = key;
                cnts[pos] = (uint8_t)count;
            }
        }
    }
}

// one lane: ctl[1], ctl[2] = cause and column of line ctl[0]
__global__ void text_cause_kernel(const uint8_t *__restrict__ text, uint64_t bytes, const u64 *__restrict__ starts, uint64_t n_lines, int k,
                                  u64 *__restrict__ ctl)
{
    const uint64_t j = ctl[0];
    if (threadIdx.x || blockIdx.x || j >= n_lines)
        return;
    const uint8_t *p = text;
    const uint64_t len = line_of(text, bytes, starts, n_lines, j, &p);
    uint64_t key = 0, col = 0;
    uint32_t count = 0;
    ctl[1] = len ? text_parse_line(p, len, k, &key, &count, &col) : 0u;
    ctl[2] = col;
}

// the lines of a text on the device, from `ws`: starts, and the scanned count of non-empty lines per 256 lines
struct TextIndex {
    u64 *starts = nullptr;
    uint64_t n_lines = 0; // the '\n' + 1: the bytes behind the last '\n' are a line, empty or not
    u64 *cnt = nullptr;
    uint64_t n_blocks = 0;
    uint64_t pairs = 0; // non-empty lines
};

// returns after `s` has been synchronised
int text_index(const uint8_t *d_text, uint64_t bytes, hipStream_t s, DevScratch &ws, TextIndex *ix)
{
    const uint64_t n_chunks = blocks_of(bytes, NL_CHUNK);
    const uint32_t aligned = (reinterpret_cast<uintptr_t>(d_text) & 15u) ? 0u : 1u;
    u64 *d_nl = nullptr, *d_sums = nullptr;
    BRX_TRY(ws.get(&d_nl, n_chunks));
    BRX_TRY(ws.get(&d_sums, keys_scan_sums(n_chunks) + 1));
    nl_count_kernel<<<grid_for(n_chunks), 256, 0, s>>>(d_text, bytes, n_chunks, aligned, d_nl);
    BRX_HIP(hipGetLastError());
    BRX_TRY(keys_scan_exclusive(d_nl, n_chunks, d_sums, s));
    u64 newlines = 0;
    BRX_HIP(hipMemcpyAsync(&newlines, d_sums + keys_scan_sums(n_chunks), 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (newlines > bytes) {
        set_error("k-mer text: %llu line ends in %llu bytes", newlines, (u64)bytes);
        return BRX_ERR_HIP;
    }
    ix->n_lines = newlines + 1;
    ix->n_blocks = blocks_of(ix->n_lines, TB);
    u64 *d_sums2 = nullptr;
    BRX_TRY(ws.get(&ix->starts, ix->n_lines));
    BRX_TRY(ws.get(&ix->cnt, ix->n_blocks));
    BRX_TRY(ws.get(&d_sums2, keys_scan_sums(ix->n_blocks) + 1));
    nl_scatter_kernel<<<grid_for(n_chunks), 256, 0, s>>>(d_text, bytes, n_chunks, aligned, d_nl, ix->starts, ix->n_lines);
    line_count_kernel<<<grid_for(ix->n_blocks), 256, 0, s>>>(d_text, bytes, ix->starts, ix->n_lines, ix->n_blocks, ix->cnt);
    BRX_HIP(hipGetLastError());
    BRX_TRY(keys_scan_exclusive(ix->cnt, ix->n_blocks, d_sums2, s));
    u64 pairs = 0;
    BRX_HIP(hipMemcpyAsync(&pairs, d_sums2 + keys_scan_sums(ix->n_blocks), 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (pairs > ix->n_lines) {
        set_error("k-mer text: %llu non-empty lines of %llu", pairs, (u64)ix->n_lines);
        return BRX_ERR_HIP;
    }
    ix->pairs = pairs;
    return BRX_OK;
}

// the pairs of the indexed lines into d_keys / d_cnts (room for ix.pairs); err3 as brx_kmertext_parse_device's.  Returns
// after `s` has been synchronised: BRX_OK, or BRX_ERR_FORMAT with err3 filled and no message set
int text_fill(const uint8_t *d_text, uint64_t bytes, const TextIndex &ix, int k, uint64_t *d_keys, uint8_t *d_cnts, uint64_t cap,
              uint64_t *err3, hipStream_t s, DevScratch &ws)
{
    u64 *d_ctl = nullptr;
    BRX_TRY(ws.get(&d_ctl, 3));
    BRX_HIP(hipMemsetAsync(d_ctl, 0xFF, 8, s));
    BRX_HIP(hipMemsetAsync(d_ctl + 1, 0, 16, s));
    text_parse_kernel<<<grid_for(ix.n_blocks), 256, 0, s>>>(d_text, bytes, ix.starts, ix.n_lines, ix.n_blocks, k, ix.cnt, d_keys, d_cnts, cap,
                                                           d_ctl);
    text_cause_kernel<<<1, 64, 0, s>>>(d_text, bytes, ix.starts, ix.n_lines, k, d_ctl);
    BRX_HIP(hipGetLastError());
    u64 ctl[3] = {0, 0, 0};
    BRX_HIP(hipMemcpyAsync(ctl, d_ctl, 24, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    err3[0] = err3[1] = err3[2] = 0;
    if (ctl[0] == NONE)
        return BRX_OK;
    err3[0] = ctl[1];
    err3[1] = ctl[0];
    err3[2] = ctl[2];
    return BRX_ERR_FORMAT;
}

// "line N: cause" in the words of br_amd/kmertext.py cause_text; line: of the whole text, from 1
void set_line_error(uint64_t line, uint64_t cause, uint64_t col, int k)
{
    const u64 n = line, c = col;
    switch (cause) {
    case TEXT_BASE: set_error("k-mer text: line %llu: column %llu is no base (ACGT, either case)", n, c); break;
    case TEXT_SHORT: set_error("k-mer text: line %llu: a k-mer of %llu bases is shorter than k=%d", n, c, k); break;
    case TEXT_LONG: set_error("k-mer text: line %llu: a k-mer of %llu bases is longer than k=%d", n, c, k); break;
    case TEXT_NOCOUNT: set_error("k-mer text: line %llu: no count after the k-mer", n); break;
    case TEXT_DIGIT: set_error("k-mer text: line %llu: column %llu is no digit", n, c); break;
    case TEXT_ZERO: set_error("k-mer text: line %llu: a count of 0", n); break;
    default: set_error("k-mer text: line %llu: malformed (cause %llu)", n, (u64)cause); break;
    }
}

bool k_ok(int k) { return (k & 1) && k >= 5 && k <= 31; }

// ---- import: order, run-sum, the list ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void descent_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    bool down = false;
    for (uint64_t i = 1 + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
        down |= keys[i] < keys[i - 1];
    if (down)
        *flag = 1u;
}

__device__ __forceinline__ bool is_head(const uint64_t *__restrict__ keys, uint64_t n, uint64_t i) { return i < n && (!i || keys[i] != keys[i - 1]); }

__global__ __launch_bounds__(256) void head_count_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n_blocks, u64 *__restrict__ cnt)
{
    __shared__ u64 sh[4];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        u64 total;
        (void)block_excl_scan(is_head(keys, n, b * TB + threadIdx.x) ? 1u : 0u, sh, &total);
        if (threadIdx.x == 0)
            cnt[b] = total;
    }
}

// cnt: scanned; m = the heads.  ctl[0]: the first output entry whose sum lies below the floor (NONE before the launch)
__global__ __launch_bounds__(256) void runsum_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ cnts, uint64_t n,
                                                     uint64_t n_blocks, const u64 *__restrict__ cnt, uint32_t floor,
                                                     uint64_t *__restrict__ out_keys, uint8_t *__restrict__ out_cnts, uint64_t m,
                                                     u64 *__restrict__ ctl)
{
    __shared__ u64 sh[4];
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) { // block-uniform
        const uint64_t i = b * TB + threadIdx.x;
        const bool head = is_head(keys, n, i);
        u64 total;
        const uint64_t pos = cnt[b] + block_excl_scan(head ? 1u : 0u, sh, &total);
        if (head && pos < m) { // (pos < m always: the heads were counted over the same keys)
            const uint64_t key = keys[i];
            uint32_t sum = cnts[i];
            for (uint64_t j = i + 1; j < n && sum < 255u && keys[j] == key; j++) // (a count is at least 1: 254 steps at most)
                sum += cnts[j];
            sum = sum > 255u ? 255u : sum;
            out_keys[pos] = key;
            out_cnts[pos] = (uint8_t)sum;
            if (sum < floor)
                atomicMin(ctl, (u64)pos);
        }
    }
}

// ctl[0]: the first index that breaks a rule of a count list (NONE before the launch)
__global__ __launch_bounds__(256) void list_check_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ cnts, uint64_t n,
                                                         uint64_t key_limit, uint32_t floor, u64 *__restrict__ ctl)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
        if (keys[i] >= key_limit || (i && keys[i] <= keys[i - 1]) || cnts[i] < floor)
            atomicMin(ctl, (u64)i);
}

// The one constructor of a list from arrays on the device (the import and brx_counts_from_arrays): n entries in buffers that
// the list takes over, checked here -- keys strictly ascending and below 2^(2k-1), counts >= floor >= 1.  *bad = NONE and
// *out = the list, or *bad = the first offending index, BRX_ERR_ARG and no message set: the caller has the words.
int counts_adopt(int k, int device, uint8_t floor, DevBuf<uint64_t> &d_keys, DevBuf<uint8_t> &d_cnts, uint64_t n, hipStream_t s, uint64_t *bad,
                 brx_counts **out)
{
    *bad = NONE;
    *out = nullptr;
    if (n) {
        DevScratch ws;
        u64 *d_ctl = nullptr;
        BRX_TRY(ws.get(&d_ctl, 1));
        BRX_HIP(hipMemsetAsync(d_ctl, 0xFF, 8, s));
        list_check_kernel<<<grid_for(blocks_of(n, TB)), 256, 0, s>>>(d_keys, d_cnts, n, set_nbits(k), floor, d_ctl);
        BRX_HIP(hipGetLastError());
        u64 first = NONE;
        BRX_HIP(hipMemcpyAsync(&first, d_ctl, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (first != NONE) {
            *bad = first;
            return BRX_ERR_ARG;
        }
    } else {
        d_keys.reset();
        d_cnts.reset();
    }
    brx_counts *l = new brx_counts;
    l->k = k;
    l->device = device;
    l->floor = floor;
    l->n = n;
    l->d_keys = std::move(d_keys);
    l->d_cnts = std::move(d_cnts);
    *out = l;
    return BRX_OK;
}

// the field of the first non-empty line of buf[0 .. len): *k = its bytes before TAB / space / line end, *line = lines in
// front of it; false: every line is empty
bool sniff_k(const uint8_t *buf, size_t len, uint64_t *k, uint64_t *line)
{
    size_t at = 0;
    for (uint64_t no = 0; at < len; no++) {
        const uint8_t *nl = (const uint8_t *)memchr(buf + at, '\n', len - at);
        const size_t end = nl ? (size_t)(nl - buf) : len;
        const size_t body = (size_t)text_trim(buf + at, end - at);
        if (body) {
            size_t f = 0;
            while (f < body && buf[at + f] != '\t' && buf[at + f] != ' ')
                f++;
            *k = f;
            *line = no;
            return true;
        }
        at = end + 1;
    }
    return false;
}

} // namespace

extern "C" {

int brx_kmertext_format_device(int k, const uint64_t *d_keys, const uint8_t *d_counts, uint64_t n, int strand, uint8_t *d_text, uint64_t cap,
                               uint64_t *bytes_out, void *stream)
{
    const char *me = "brx_kmertext_format_device";
    if (!bytes_out || !k_ok(k) || (strand != BRX_TEXT_LEX && strand != BRX_TEXT_CANONICAL) || (n && (!d_keys || !d_counts))) {
        set_error("%s: null bytes_out / keys / counts, k=%d (odd k from 5 to 31) or strand=%d (BRX_TEXT_LEX, BRX_TEXT_CANONICAL)", me, k, strand);
        return BRX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    *bytes_out = 0;
    if (!n) {
        BRX_HIP(hipStreamSynchronize(s));
        return BRX_OK;
    }
    const uint64_t nb = blocks_of(n, TB);
    DevScratch ws;
    u64 *d_size = nullptr, *d_sums = nullptr;
    BRX_TRY(ws.get(&d_size, nb));
    BRX_TRY(ws.get(&d_sums, keys_scan_sums(nb) + 1));
    int st;
    u64 total = 0;
    {
        KernelTimer kt("text_format", s);
        st = format_measure(k, d_counts, n, d_size, d_sums, s);
    }
    if (st != BRX_OK) {
        (void)hipStreamSynchronize(s); // the scratch goes back to the pool below
        return st;
    }
    BRX_HIP(hipMemcpyAsync(&total, d_sums + keys_scan_sums(nb), 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (total > n * (uint64_t)(k + 5)) {
        set_error("%s: %llu bytes for %llu entries", me, total, (u64)n);
        return BRX_ERR_HIP;
    }
    *bytes_out = total;
    if (total > cap || !d_text) {
        set_error("%s: the text takes %llu bytes, d_text holds %llu", me, total, (u64)(d_text ? cap : 0));
        return BRX_ERR_ARG;
    }
    {
        KernelTimer kt("text_format", s);
        st = format_write(k, d_keys, d_counts, n, strand, d_size, total, d_text, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    if (st == BRX_OK && e2 != hipSuccess) {
        set_error("%s: writing: %s", me, hipGetErrorString(e2));
        return BRX_ERR_HIP;
    }
    return st;
}

int brx_kmertext_parse_device(const uint8_t *d_text, uint64_t bytes, int k, uint64_t *d_keys, uint8_t *d_counts, uint64_t cap, uint64_t *n_out,
                              uint64_t *err3, void *stream)
{
    const char *me = "brx_kmertext_parse_device";
    if (!n_out || !err3 || !k_ok(k) || (bytes && !d_text)) {
        set_error("%s: null n_out / err3 / text, or k=%d (odd k from 5 to 31)", me, k);
        return BRX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    *n_out = 0;
    err3[0] = err3[1] = err3[2] = 0;
    if (!bytes) {
        BRX_HIP(hipStreamSynchronize(s));
        return BRX_OK;
    }
    DevScratch ws;
    TextIndex ix;
    int st;
    {
        KernelTimer kt("text_parse", s);
        st = text_index(d_text, bytes, s, ws, &ix);
    }
    if (st != BRX_OK) {
        (void)hipStreamSynchronize(s);
        return st;
    }
    if (ix.pairs > cap || (ix.pairs && (!d_keys || !d_counts))) {
        *n_out = ix.pairs;
        set_error("%s: %llu non-empty lines, the outputs hold %llu", me, (u64)ix.pairs, (u64)((d_keys && d_counts) ? cap : 0));
        return BRX_ERR_ARG;
    }
    {
        KernelTimer kt("text_parse", s);
        st = text_fill(d_text, bytes, ix, k, d_keys, d_counts, cap, err3, s, ws);
    }
    if (st == BRX_ERR_FORMAT)
        set_line_error(err3[1] + 1, err3[0], err3[2], k);
    if (st != BRX_OK) {
        (void)hipStreamSynchronize(s);
        return st;
    }
    *n_out = ix.pairs;
    return BRX_OK;
}

int brx_counts_dump_text_fd(const brx_counts_t *l, uint8_t min_count, int strand, int out_fd, uint64_t *stats8)
{
    const char *me = "brx_counts_dump_text_fd";
    BRX_TRY(list_ok(me, l));
    if (out_fd < 0 || (strand != BRX_TEXT_LEX && strand != BRX_TEXT_CANONICAL)) {
        set_error("%s: bad descriptor, or strand=%d (BRX_TEXT_LEX, BRX_TEXT_CANONICAL)", me, strand);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(l->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    const uint64_t *d_keys = l->d_keys;
    const uint8_t *d_cnts = l->d_cnts;
    uint64_t n = l->n;
    DevBuf<uint64_t> d_kept;
    DevBuf<uint8_t> d_kept_cnts;
    if (min_count > l->floor) { // one compaction, as brx_counts_save_fd does it
        BRX_TRY(counts_merge(me, l->d_keys, l->d_cnts, l->n, nullptr, nullptr, 0, BRX_COUNTOP_ADD, min_count, true, s, d_kept, d_kept_cnts, &n,
                             nullptr));
        d_keys = d_kept;
        d_cnts = d_kept_cnts;
        st8[4] = ns_since(t0);
    }
    const int k = l->k;
    const size_t piece = slice_bytes();
    const uint64_t per = piece / (size_t)(k + 6); // entries of a slice: their lines fit a piece
    const uint64_t n_slices = blocks_of(n, (uint32_t)per);
    uint64_t total = 0, ns_fd = 0;
    auto t1 = Clock::now();
    auto run = [&]() -> int {
        if (!n)
            return BRX_OK;
        PinnedPair pin;
        EventPair ev;
        DevScratch ws;
        uint8_t *d_text = nullptr;
        u64 *d_size = nullptr, *d_sums = nullptr, *d_slice = nullptr;
        const uint64_t nb_max = blocks_of(per, TB);
        BRX_TRY(pin.get(piece));
        BRX_TRY(ev.make());
        BRX_TRY(ws.get(&d_text, piece));
        BRX_TRY(ws.get(&d_size, nb_max));
        BRX_TRY(ws.get(&d_sums, keys_scan_sums(nb_max) + 1));
        BRX_TRY(ws.get(&d_slice, n_slices));
        std::vector<u64> len(n_slices);
        {
            KernelTimer kt("text_format", s);
            text_slice_sizes_kernel<<<grid_for(n_slices), 256, 0, s>>>(d_cnts, n, per, n_slices, k, d_slice);
            BRX_HIP(hipGetLastError());
        }
        BRX_HIP(hipMemcpyAsync(len.data(), d_slice, n_slices * 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < n_slices; i++)
            if (len[i] > piece) {
                set_error("%s: slice %llu takes %llu bytes, a piece holds %llu", me, (u64)i, len[i], (u64)piece);
                return BRX_ERR_HIP;
            }
        // slice i: formatted into the device piece, copied into page-locked piece i & 1; everything in the order of `s`
        auto start = [&](uint64_t i) -> int {
            const uint64_t e0 = i * per, m = n - e0 < per ? n - e0 : per;
            {
                KernelTimer kt("text_format", s);
                BRX_TRY(format_measure(k, d_cnts + e0, m, d_size, d_sums, s));
                BRX_TRY(format_write(k, d_keys + e0, d_cnts + e0, m, strand, d_size, len[i], d_text, s));
            }
            BRX_HIP(hipMemcpyAsync(pin.p[i & 1], d_text, len[i], hipMemcpyDeviceToHost, s));
            BRX_HIP(hipEventRecord(ev.e[i & 1], s));
            return BRX_OK;
        };
        int st = start(0);
        for (uint64_t i = 0; i < n_slices && st == BRX_OK; i++) {
            if (i + 1 < n_slices) // (its page-locked piece was written out in the trip before): formatted while slice i is written
                st = start(i + 1);
            if (st != BRX_OK)
                break;
            if (hipEventSynchronize(ev.e[i & 1]) != hipSuccess) {
                set_error("%s: copy of slice %llu failed", me, (u64)i);
                st = BRX_ERR_HIP;
                break;
            }
            auto tw = Clock::now();
            st = write_all(out_fd, pin.p[i & 1], (size_t)len[i]);
            ns_fd += ns_since(tw);
            total += len[i];
        }
        (void)hipStreamSynchronize(s); // nothing may still be copying into the pieces when they are released
        return st;
    };
    const int st = run();
    st8[0] = n;
    st8[1] = total;
    st8[2] = n_slices;
    st8[6] = ns_fd;
    st8[5] = ns_since(t1) - ns_fd;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return st;
}

int brx_counts_from_arrays(int k, const uint64_t *keys, const uint8_t *counts, uint64_t n, uint8_t floor, int device, brx_counts_t **out)
{
    const char *me = "brx_counts_from_arrays";
    if (!out || !k_ok(k) || (n && (!keys || !counts))) {
        set_error("%s: null out / keys / counts, or k=%d (odd k from 5 to 31)", me, k);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    if (floor < 1)
        floor = 1;
    BRX_TRY(use_device(device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    DevBuf<uint64_t> d_keys;
    DevBuf<uint8_t> d_cnts;
    if (n) {
        BRX_TRY(d_keys.reserve(n, 0, "keys of a count list"));
        BRX_TRY(d_cnts.reserve(n, 0, "counts of a count list"));
        BRX_HIP(hipMemcpyAsync(d_keys, keys, n * 8, hipMemcpyHostToDevice, own.s));
        BRX_HIP(hipMemcpyAsync(d_cnts, counts, n, hipMemcpyHostToDevice, own.s));
    }
    uint64_t bad = NONE;
    const int st = counts_adopt(k, device, floor, d_keys, d_cnts, n, own.s, &bad, out);
    if (st == BRX_ERR_ARG && bad != NONE && bad < n) {
        const u64 i = bad;
        if (keys[i] >= set_nbits(k))
            set_error("%s: index %llu: key %llu is not below 2^%d (k=%d)", me, i, (u64)keys[i], 2 * k - 1, k);
        else if (i && keys[i] <= keys[i - 1])
            set_error("%s: index %llu: key %llu does not exceed the key before it (%llu): keys ascend strictly", me, i, (u64)keys[i],
                      (u64)keys[i - 1]);
        else
            set_error("%s: index %llu: count %d is below the floor %d", me, i, (int)counts[i], (int)floor);
    }
    return st;
}

int brx_counts_import_text_fd(int in_fd, int k, uint8_t floor, int device, brx_counts_t **out, uint64_t *stats8)
{
    const char *me = "brx_counts_import_text_fd";
    if (!out || in_fd < 0 || (k && !k_ok(k))) {
        set_error("%s: null out, bad descriptor, or k=%d (0: from the first line; odd k from 5 to 31)", me, k);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    if (floor < 1)
        floor = 1;
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    const size_t piece = slice_bytes();
    PinnedPair pin;
    DevBuf<uint8_t> d_text;
    DevBuf<uint64_t> acc_k;
    DevBuf<uint8_t> acc_c;
    uint64_t acc_n = 0, acc_cap = 0, line0 = 0, text_bytes = 0, ns_fd = 0;
    BRX_TRY(pin.get(piece));
    BRX_TRY(d_text.reserve(piece, 0, "a piece of k-mer text"));
    // ---- the pieces: each cut at its last line end, the rest carried in front of the next one
    size_t carry = 0;
    for (int cur = 0;; cur ^= 1) {
        uint8_t *buf = pin.p[cur];
        size_t got = 0;
        auto tr = Clock::now();
        BRX_TRY(read_upto(in_fd, buf + carry, piece - carry, &got));
        ns_fd += ns_since(tr);
        const bool eof = got < piece - carry;
        const size_t have = carry + got;
        text_bytes += got;
        if (!have)
            break;
        size_t cut = have; // (the end of the text is the end of its last line)
        if (!eof) {
            const uint8_t *nl = (const uint8_t *)memrchr(buf, '\n', have);
            if (!nl) {
                set_error("k-mer text: line %llu: longer than a piece of %llu bytes (BRX_KEYFILE_SLICE_KB)", (u64)line0 + 1, (u64)piece);
                return BRX_ERR_FORMAT;
            }
            cut = (size_t)(nl - buf) + 1;
        }
        if (!k) {
            uint64_t field = 0, before = 0;
            if (sniff_k(buf, cut, &field, &before)) {
                if (!(field & 1) || field < 5 || field > 31) {
                    set_error("k-mer text: line %llu: a k-mer of %llu bases gives no k (odd, 5 to 31)", (u64)(line0 + before + 1), (u64)field);
                    return BRX_ERR_FORMAT;
                }
                k = (int)field;
            }
        }
        BRX_HIP(hipMemcpyAsync(d_text, buf, cut, hipMemcpyHostToDevice, s));
        {
            DevScratch ws;
            TextIndex ix;
            int st;
            {
                KernelTimer kt("text_parse", s);
                st = text_index(d_text, cut, s, ws, &ix);
            }
            if (st == BRX_OK && k && ix.pairs) {
                if (acc_n + ix.pairs > acc_cap) { // grow geometrically; the pairs so far move over
                    const uint64_t want = acc_n + ix.pairs > 2 * acc_cap ? acc_n + ix.pairs : 2 * acc_cap;
                    DevBuf<uint64_t> nk;
                    DevBuf<uint8_t> nc;
                    BRX_TRY(nk.reserve(want, 0, "keys of a k-mer text"));
                    BRX_TRY(nc.reserve(want, 0, "counts of a k-mer text"));
                    if (acc_n) {
                        BRX_HIP(hipMemcpyAsync(nk, acc_k, acc_n * 8, hipMemcpyDeviceToDevice, s));
                        BRX_HIP(hipMemcpyAsync(nc, acc_c, acc_n, hipMemcpyDeviceToDevice, s));
                        BRX_HIP(hipStreamSynchronize(s));
                    }
                    acc_k = std::move(nk);
                    acc_c = std::move(nc);
                    acc_cap = want;
                }
                uint64_t err3[3];
                {
                    KernelTimer kt("text_parse", s);
                    st = text_fill(d_text, cut, ix, k, acc_k.get() + acc_n, acc_c.get() + acc_n, ix.pairs, err3, s, ws);
                }
                if (st == BRX_ERR_FORMAT)
                    set_line_error(line0 + err3[1] + 1, err3[0], err3[2], k);
                acc_n += ix.pairs;
            }
            (void)hipStreamSynchronize(s); // the scratch goes back to the pool below
            if (st != BRX_OK)
                return st;
            line0 += ix.n_lines - 1; // (a piece that is cut ends at a line end; the last one ends the text)
        }
        carry = have - cut;
        if (carry)
            memcpy(pin.p[cur ^ 1], buf + cut, carry);
        if (eof)
            break;
    }
    if (!k) {
        set_error("k-mer text: an empty text tells no k");
        return BRX_ERR_FORMAT;
    }
    st8[5] = ns_since(t0) - ns_fd;
    st8[6] = ns_fd;
    st8[1] = text_bytes;
    st8[2] = acc_n;
    d_text.reset();
    // ---- sort where the keys ever descend, sum the runs of equal keys, check the floor
    auto t1 = Clock::now();
    DevBuf<uint64_t> d_keys;
    DevBuf<uint8_t> d_cnts;
    uint64_t m = 0;
    if (acc_n) {
        DevScratch ws;
        const uint64_t nb = blocks_of(acc_n, TB);
        u64 *d_ctl = nullptr, *d_heads = nullptr, *d_sums = nullptr; // ctl[0]: first entry below the floor; [1]: descent flag
        BRX_TRY(ws.get(&d_ctl, 2));
        BRX_TRY(ws.get(&d_heads, nb));
        BRX_TRY(ws.get(&d_sums, keys_scan_sums(nb) + 1));
        BRX_HIP(hipMemsetAsync(d_ctl, 0xFF, 8, s));
        BRX_HIP(hipMemsetAsync(d_ctl + 1, 0, 8, s));
        {
            KernelTimer kt("text_parse", s);
            descent_kernel<<<grid_for(nb), 256, 0, s>>>(acc_k, acc_n, (uint32_t *)(d_ctl + 1));
            BRX_HIP(hipGetLastError());
        }
        u64 down = 0;
        BRX_HIP(hipMemcpyAsync(&down, d_ctl + 1, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (down) {
            st8[3] = 1;
            BRX_TRY(keys_sort(acc_k, acc_c, acc_n, (uint32_t)(2 * k - 1), s));
        }
        u64 heads = 0;
        {
            KernelTimer kt("text_runsum", s);
            head_count_kernel<<<grid_for(nb), 256, 0, s>>>(acc_k, acc_n, nb, d_heads);
            BRX_HIP(hipGetLastError());
            BRX_TRY(keys_scan_exclusive(d_heads, nb, d_sums, s));
        }
        BRX_HIP(hipMemcpyAsync(&heads, d_sums + keys_scan_sums(nb), 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (!heads || heads > acc_n) {
            set_error("%s: %llu distinct keys among %llu pairs", me, heads, (u64)acc_n);
            return BRX_ERR_HIP;
        }
        m = heads;
        BRX_TRY(d_keys.reserve(m, 0, "keys of a count list"));
        BRX_TRY(d_cnts.reserve(m, 0, "counts of a count list"));
        {
            KernelTimer kt("text_runsum", s);
            runsum_kernel<<<grid_for(nb), 256, 0, s>>>(acc_k, acc_c, acc_n, nb, d_heads, floor, d_keys, d_cnts, m, d_ctl);
            BRX_HIP(hipGetLastError());
        }
        u64 low = NONE;
        BRX_HIP(hipMemcpyAsync(&low, d_ctl, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (low != NONE && low < m) {
            u64 key = 0;
            uint8_t c = 0;
            BRX_HIP(hipMemcpy(&key, d_keys.get() + low, 8, hipMemcpyDeviceToHost));
            BRX_HIP(hipMemcpy(&c, d_cnts.get() + low, 1, hipMemcpyDeviceToHost));
            set_error("k-mer text: the k-mer of key %llu is counted %d times in all, below the floor %d", key, (int)c, (int)floor);
            return BRX_ERR_FORMAT;
        }
        acc_k.reset();
        acc_c.reset();
    }
    uint64_t bad = NONE;
    const int st = counts_adopt(k, device, floor, d_keys, d_cnts, m, s, &bad, out);
    if (st == BRX_ERR_ARG && bad != NONE) {
        set_error("%s: entry %llu of the summed list breaks the rules of a count list", me, (u64)bad);
        return BRX_ERR_HIP;
    }
    st8[4] = ns_since(t1);
    st8[0] = m;
    st8[7] = ns_since(t0);
    if (st == BRX_OK && stats8)
        memcpy(stats8, st8, sizeof st8);
    return st;
}

} // extern "C"
