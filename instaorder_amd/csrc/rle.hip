// Run-length-encoded instance masks -> dense uint8 masks, on the device (DESIGN.md "Run-length masks").
//
// The format is COCO's: the pixels of an H x W mask in COLUMN-major order (q = x * H + y) as alternating runs of 0 and 1,
// starting with a run of zeros; zero-length runs may appear anywhere.  The host ships, per mask, the inclusive prefix sums
// `ends` of the run lengths (uint32), and pixel q lies in run r = #{k : ends[k] <= q} (an upper bound), value r & 1.
// Repeated entries of `ends` (zero-length runs) need no special case under that rule.
//
// The consumers (pair_planes_kernel, io_mask_pack) read ROW-major masks, so this is a search per output pixel, not a fill
// per run: a thread owns one aligned 4-byte word of the output, walks its four pixels (q grows by H along a row, so the
// search of a pixel starts at the run of the pixel before it) and stores the word once.  The run table of a mask is staged
// in LDS when it has at most IO_RLE_LDS_RUNS entries -- every search step is then a 4-byte LDS read -- and searched in
// global memory (L2-resident: a table is read by all blocks of its mask) when it is longer.
//
// Safety does not depend on the table's contents: the search reads indices in [0, n_runs) only, its result only selects
// one of two byte values, and every store address comes from the descriptor the host validated.
#include "io_common.h"

namespace {

constexpr int kThreads = 256;                // four wave64
constexpr int kWordsPerThread = 4;           // 16 output pixels per thread and chunk
constexpr int kChunkWords = kThreads * kWordsPerThread;

// r = #{k in [lo, n) : ends[k] <= q} + lo; reads ends[lo .. n) only
template <typename Ptr>
__device__ __forceinline__ int upper_bound_from(Ptr ends, int lo, int n, unsigned q) {
    int hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (ends[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the (up to) four pixels p0 .. p0 + 3 of the row-major mask, those inside [0, HW) only; byte k of the result = pixel p0 + k
template <typename Ptr>
__device__ __forceinline__ unsigned decode_word(Ptr ends, int n_runs, int H, int W, long p0, long HW, unsigned value) {
    const int k0 = p0 < 0 ? (int)-p0 : 0;                 // first pixel of the word inside the mask (p0 >= -3)
    const unsigned first = (unsigned)(p0 + k0);
    int y = (int)(first / (unsigned)W);                   // one division per word; the walk below carries (y, x) on
    int x = (int)first - y * W;
    unsigned word = 0;
    int r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < k0 || p0 + k >= HW) continue;
        const unsigned q = (unsigned)x * (unsigned)H + (unsigned)y;
        // along a row q only grows, so (for a well-formed table) the run index cannot fall below the previous pixel's;
        // r is reset where the walk wraps to the next row
        r = upper_bound_from(ends, r, n_runs, q);
        if (r & 1) word |= value << (8 * k);
        if (++x == W) { x = 0; ++y; r = 0; }
    }
    return word;
}

__global__ __launch_bounds__(kThreads) void rle_decode_kernel(const uint32_t* __restrict__ ends_all,
                                                              const io_rle_desc* __restrict__ desc,
                                                              uint8_t* __restrict__ out) {
    __shared__ uint32_t s_ends[IO_RLE_LDS_RUNS];
    const io_rle_desc d = desc[blockIdx.y];
    const long HW = (long)d.H * d.W;
    uint8_t* dst = out + d.out_off;
    // aligned 4-byte words that cover dst[0 .. HW): word w holds the pixels 4 * w - head .. 4 * w - head + 3
    const int head = (int)((uintptr_t)dst & 3);
    const long nwords = (HW + head + 3) >> 2;
    // grid.x = chunks of the largest mask of the launch; a smaller mask leaves its last blocks idle
    if ((long)blockIdx.x * kChunkWords >= nwords) return;   // block-uniform: nobody is left behind at the barrier below
    const uint32_t* ends = ends_all + d.ends_off;
    const bool staged = d.n_runs <= IO_RLE_LDS_RUNS;
    if (staged) {
        for (int k = threadIdx.x; k < d.n_runs; k += kThreads) s_ends[k] = ends[k];
        __syncthreads();
    }
    const unsigned value = (unsigned)d.value & 0xffu;
#pragma unroll
    for (int j = 0; j < kWordsPerThread; ++j) {
        // consecutive lanes write consecutive words: 256 B per wave and store
        const long w = (long)blockIdx.x * kChunkWords + j * kThreads + threadIdx.x;
        if (w >= nwords) break;
        const long p0 = 4 * w - head;
        const unsigned word = staged ? decode_word(s_ends, d.n_runs, d.H, d.W, p0, HW, value)
                                     : decode_word(ends, d.n_runs, d.H, d.W, p0, HW, value);
        if (p0 >= 0 && p0 + 4 <= HW) {
            *reinterpret_cast<uint32_t*>(dst + p0) = word;
        } else {                                        // first / last word of a mask: bytes outside it are not ours
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= 0 && p0 + k < HW) dst[p0 + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

}  // namespace

extern "C" int io_rle_lds_runs(void) { return IO_RLE_LDS_RUNS; }

extern "C" int io_rle_decode_u8(const uint32_t* ends_dev, size_t ends_count, const io_rle_desc* desc_dev,
                                const io_rle_desc* desc_host, int n, uint8_t* out, size_t out_bytes, hipStream_t st) {
    IO_REQUIRE(n > 0 && ends_dev && desc_dev && desc_host && out, IO_ERR_SHAPE,
               "rle_decode: empty batch or null pointer (n=%d)", n);
    IO_REQUIRE(n <= 65535, IO_ERR_SHAPE, "rle_decode: n=%d out of range (at most 65535 masks per launch)", n);
    // the descriptors are validated on the host copy: every entry the kernel may read lies inside the table buffer and
    // every byte it may write inside `out`
    double table_bytes = 0.0, pixels = 0.0;
    long max_words = 0;
    for (int i = 0; i < n; ++i) {
        const io_rle_desc& d = desc_host[i];
        IO_REQUIRE(d.H > 0 && d.W > 0 && (long)d.H * d.W < (1L << 31), IO_ERR_SHAPE,
                   "rle_decode: mask %d has size %d x %d (need H, W > 0 and H * W < 2^31)", i, d.H, d.W);
        IO_REQUIRE(d.n_runs >= 1, IO_ERR_SHAPE, "rle_decode: mask %d has n_runs=%d (at least one run)", i, d.n_runs);
        IO_REQUIRE(d.value >= 0 && d.value <= 255, IO_ERR_SHAPE, "rle_decode: mask %d value=%d does not fit a byte", i,
                   d.value);
        IO_REQUIRE(d.ends_off >= 0 && (size_t)d.ends_off <= ends_count &&
                       (size_t)d.n_runs <= ends_count - (size_t)d.ends_off,
                   IO_ERR_SHAPE, "rle_decode: mask %d run table outside the table buffer", i);
        const size_t hw = (size_t)d.H * (size_t)d.W;
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && hw <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "rle_decode: mask %d output outside the output buffer", i);
        table_bytes += 4.0 * d.n_runs;
        pixels += (double)hw;
        const long words = ((long)hw + 3 + 3) / 4;
        if (words > max_words) max_words = words;
    }
    const int gx = io_cdiv(max_words, kChunkWords);      // < 2^19 for H * W < 2^31
    IoProfScope prof(IO_PROF_RLE, 0.0, table_bytes + pixels, st);
    hipLaunchKernelGGL(rle_decode_kernel, dim3(gx, n), dim3(kThreads), 0, st, ends_dev, desc_dev, out);
    return io_check_launch("rle_decode");
}
