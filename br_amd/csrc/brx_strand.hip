// Reverse complement of reads on the device: the byte map between the two scans of a chain in BRX_PASS_REVCOMP mode
// (brx_correct.hip) and the entry points brx_revcomp_batch[_device].
//
// rc(s) is the bytes of s in reverse order with A<->T, C<->G, a<->t, c<->g exchanged; every other byte stays.  The
// reference has no such step: its second scan reverses and does not complement (src/lib.rs:111).
//
// One kernel in three forms (where a read starts on either side: the batch's offsets, or its staging slot):
//   staged -> staged    between the scans: the other staging buffer, same slot layout, lengths carried over
//   staged -> compact   after the second scan, into the output (the sibling of compact_kernel)
//   batch  -> batch     brx_revcomp_batch_device
// Shaped like compact_kernel: one workgroup per read (grid-stride), destination-aligned 16-byte stores, one unaligned
// 16-byte load at the mirrored address, byte order turned in registers, the complement on the four 32-bit words with
// integer masks.  No table, no LDS.
#include "brx_correct.hpp"

namespace brx {
namespace {

// 0x80 in every byte of x that is NOT zero (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// complement of four bases at once.  A ^ T = a ^ t = 0x15 and C ^ G = c ^ g = 0x04, so a letter becomes its partner by
// one XOR; with bit 5 (the case) cleared A = 0x41, T = 0x54, and C / G = 0x43 / 0x47 differ in bit 2 alone.
__device__ __forceinline__ uint32_t comp4(uint32_t w)
{
    const uint32_t u = w & 0xdfdfdfdfu;
    const uint32_t at = (~(nonzero_bytes(u ^ 0x41414141u) & nonzero_bytes(u ^ 0x54545454u)) & 0x80808080u) >> 7;
    const uint32_t cg = (~nonzero_bytes((u & 0xfbfbfbfbu) ^ 0x43434343u) & 0x80808080u) >> 7;
    return w ^ (at | (at << 2) | (at << 4)) ^ (cg << 2);
}

__device__ __forceinline__ uint8_t comp1(uint8_t b)
{
    return (uint8_t)comp4(b); // (the three zero bytes above it are no letters and stay zero)
}

template <bool SRC_STAGED, bool DST_STAGED>
__global__ __launch_bounds__(256) void revcomp_kernel(const uint8_t *__restrict__ in, const uint32_t *__restrict__ in_lens,
                                                      const uint64_t *__restrict__ offsets, uint32_t n_reads, uint32_t slack,
                                                      const uint64_t *__restrict__ out_offsets, uint8_t *__restrict__ out,
                                                      uint32_t *__restrict__ out_lens)
{
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t o0 = offsets[r], o1 = offsets[r + 1];
        const uint64_t s0 = slot_of(o0, r, slack);
        const uint8_t *src = in + (SRC_STAGED ? s0 : o0);
        uint32_t n = SRC_STAGED ? in_lens[r] : (uint32_t)(o1 - o0);
        if (SRC_STAGED) {
            if (DST_STAGED && n == 0xffffffffu) { // given up by a pass of the first scan: stays poisoned, nothing to turn
                if (threadIdx.x == 0)
                    out_lens[r] = 0xffffffffu;
                continue;
            }
            // (compact_kernel's rule: a read redone outside the batch may have its length here and its bytes elsewhere)
            const uint64_t slot = slot_of(o1, (uint64_t)r + 1, slack) - s0;
            if ((uint64_t)n > slot)
                n = (uint32_t)slot;
        }
        uint8_t *dst = out + (DST_STAGED ? s0 : out_offsets[r]);
        if (DST_STAGED && threadIdx.x == 0)
            out_lens[r] = n;
        // bytes up to the first 16-byte boundary of dst, then 16 bytes per lane (unaligned load at the mirrored address,
        // byte order turned and bases complemented in registers, aligned store), then the tail
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
        if (head > n)
            head = n;
        const uint32_t nv = (n - head) / 16u;
        for (uint32_t j = threadIdx.x; j < head; j += blockDim.x)
            dst[j] = comp1(src[n - 1u - j]);
        for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
            const uint32_t j = head + 16u * v;
            uint4 q;
            __builtin_memcpy(&q, src + (n - 16u - j), 16);
            q = make_uint4(comp4(__builtin_bswap32(q.w)), comp4(__builtin_bswap32(q.z)), comp4(__builtin_bswap32(q.y)),
                           comp4(__builtin_bswap32(q.x)));
            *reinterpret_cast<uint4 *>(dst + j) = q;
        }
        for (uint32_t j = head + 16u * nv + threadIdx.x; j < n; j += blockDim.x)
            dst[j] = comp1(src[n - 1u - j]);
    }
}

inline uint32_t grid_of(uint32_t n_reads) { return read_grid(n_reads, 1u << 20); }

} // namespace

void revcomp_stage(const uint8_t *stage_in, const uint32_t *lens_in, const uint64_t *d_offsets, uint32_t n_reads, uint32_t slack,
                   uint8_t *stage_out, uint32_t *lens_out, hipStream_t s)
{
    KernelTimer t("strand", s);
    revcomp_kernel<true, true><<<grid_of(n_reads), 256, 0, s>>>(stage_in, lens_in, d_offsets, n_reads, slack, nullptr, stage_out, lens_out);
}

void revcomp_compact(const uint8_t *stage, const uint32_t *lens, const uint64_t *d_offsets, uint32_t n_reads, uint32_t slack,
                     const uint64_t *d_out_offsets, uint8_t *d_out, hipStream_t s)
{
    KernelTimer t("strand_compact", s);
    revcomp_kernel<true, false><<<grid_of(n_reads), 256, 0, s>>>(stage, lens, d_offsets, n_reads, slack, d_out_offsets, d_out, nullptr);
}

void revcomp_host(uint8_t *p, size_t n)
{
    static const struct Table {
        uint8_t t[256];
        Table()
        {
            for (int i = 0; i < 256; i++)
                t[i] = (uint8_t)i;
            const char *a = "ACGTacgt", *b = "TGCAtgca";
            for (int i = 0; a[i]; i++)
                t[(uint8_t)a[i]] = (uint8_t)b[i];
        }
    } tab;
    for (size_t i = 0, j = n; i < j--; i++) {
        const uint8_t x = tab.t[p[i]], y = tab.t[p[j]];
        p[i] = y;
        p[j] = x;
    }
}

} // namespace brx

using namespace brx;

extern "C" {

int brx_revcomp_batch_device(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                             uint8_t *d_out, void *stream)
{
    if (!d_offsets || (total_bases && (!d_bases || !d_out))) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    if (d_out && d_out == d_bases) {
        set_error("brx_revcomp_batch_device: d_out must not alias d_bases");
        return BRX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_reads && total_bases) {
        KernelTimer t("strand", s);
        revcomp_kernel<false, false><<<grid_of(n_reads), 256, 0, s>>>(d_bases, nullptr, d_offsets, n_reads, 0, d_offsets, d_out, nullptr);
    }
    BRX_HIP(hipGetLastError());
    BRX_HIP(hipStreamSynchronize(s));
    return BRX_OK;
}

int brx_revcomp_batch(const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint8_t *out, int device)
{
    if (!offsets || (n_reads && offsets[n_reads] && (!bases || !out))) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    BRX_TRY(use_device(device));
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    BRX_TRY(check_offsets("brx_revcomp_batch", offsets, n_reads, true));
    if (total == 0)
        return BRX_OK;
    DevBuf<uint8_t> d_in, d_o;
    DevBuf<uint64_t> d_off;
    BRX_TRY(d_in.reserve(total, 0, "reads"));
    BRX_TRY(d_o.reserve(total, 0, "reverse complements"));
    BRX_TRY(d_off.reserve((uint64_t)n_reads + 1, 0, "offsets"));
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_in, bases, total, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_off, offsets, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s);
    // (bytes of `bases` in front of offsets[0] belong to no read: `out` keeps what it held there)
    int st = BRX_OK;
    if (e == hipSuccess) {
        st = brx_revcomp_batch_device(d_in, d_off, n_reads, total, d_o, s);
        if (st == BRX_OK && total > offsets[0])
            e = hipMemcpyAsync(out + offsets[0], d_o + offsets[0], total - offsets[0], hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        set_error("brx_revcomp_batch: %s", hipGetErrorString(e));
        st = e == hipErrorOutOfMemory ? BRX_ERR_NOMEM : BRX_ERR_HIP;
    }
    if (s)
        (void)hipStreamDestroy(s);
    return st;
}

} // extern "C"
