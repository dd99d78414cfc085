// PNG images decoded on the device (DESIGN.md "PNG images"): io_png_decode.  The host parses the chunks (instaorder_amd/
// png.py); what arrives is the DEFLATE bytes of every image in one pool and one descriptor per image.  Stages, one launch
// each behind an offset launch, all on the caller's stream:
//   1. png_inflate_kernel   one wave per image: csrc/png_inflate.h (uniform symbol loop, tables and a 32 KiB ring of the
//                           output in LDS, matches copied ring to ring by all lanes, whole-wave flushes) writes the
//                           filtered scanlines, H * (1 + rowbytes) bytes, to the image's workspace range.
//      png_adler_kernel     one block per image: Adler-32 of those bytes against the descriptor's word.
//   2. png_unfilter_kernel  one wave per image, in place: a skewed wavefront over bands of PNG_BAND_ROWS rows.  Lane r takes
//                           row y0 + r and trails lane r - 1 by one pixel, so "above" is that lane's result of the step
//                           before (one lane shift) and "above left" the value it had the step before that; all bpp bytes
//                           of a pixel go in one step and each lane applies its own row's filter type.  A band costs
//                           W + 63 steps.  Lane 0 reads the last row of the band before from memory.
//   3. png_pack_kernel      as jpeg_colour_kernel: a thread owns one aligned 4-byte word of the output and gathers its
//                           (at most 4) bytes: RGB copied, alpha dropped, gray replicated, raw16 swapped to host order.
// A kernel behind a failed stage leaves the image alone (status word not zero).  Every loop bound follows from the
// descriptor: see png_inflate.h for stage 1; the others run over H, W and the output size.
//
// io_png_decode_par (opt-in, DESIGN.md "Parallel inflate") replaces stage 1 by the rule of csrc/png_inflate_par.h: ONE stream
// on many waves from found block starts.  One launch per step, every cross-chunk dependency a kernel boundary, no workgroup
// ever waits for another: png_par_search_kernel and png_par_count_kernel (a wave per chunk), png_par_chain_kernel (a lane per
// image), png_par_store_kernel (a wave per chain chunk, 16-bit symbols), png_par_tail_kernel (window propagation, a workgroup
// per image), png_par_head_kernel (every other symbol independently) and png_inflate_pred_kernel, the sequential stage
// under a per-image predicate for everything that is not a clean chain of two chunks or more.  Stages 2 and 3 run unchanged.
#include "io_common.h"
#include "png_inflate.h"
#include "png_inflate_par.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWordsPerThread = 4;
constexpr int kChunkWords = kThreads * kWordsPerThread;
#define PNG_BAND_ROWS 64

__host__ __device__ inline long png_rowbytes(const io_png_desc& d) { return (long)d.W * d.channels * (d.depth >> 3); }
__host__ __device__ inline long png_inflated(const io_png_desc& d) { return (long)d.H * (1 + png_rowbytes(d)); }
__host__ __device__ inline long png_out_bytes(const io_png_desc& d) { return (long)d.H * d.W * (d.depth == 16 ? 2 : 3); }

// off[i]: first 16-byte unit of image i's scanlines in the workspace behind the offsets
__global__ void png_offsets_kernel(const io_png_desc* __restrict__ desc, int n, unsigned long long* __restrict__ off) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long at = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = at;
        at += (unsigned long long)((png_inflated(desc[i]) + 15) >> 4);
    }
    off[n] = at;
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ pool, const io_png_desc* __restrict__ desc,
                                                         const unsigned long long* __restrict__ off, uint8_t* __restrict__ lines,
                                                         int32_t* __restrict__ status) {
    __shared__ PngShared sh;
    const io_png_desc d = desc[blockIdx.x];
    const int rc = png_inflate(&sh, pool + d.data_off, d.data_bytes, lines + 16 * (long)off[blockIdx.x], png_inflated(d),
                               (int)threadIdx.x, 64);
    if (threadIdx.x == 0) status[blockIdx.x] = rc;
}

__global__ __launch_bounds__(kThreads) void png_adler_kernel(const io_png_desc* __restrict__ desc,
                                                             const unsigned long long* __restrict__ off,
                                                             const uint8_t* __restrict__ lines, int32_t* __restrict__ status) {
    __shared__ unsigned long long r1[kThreads], r2[kThreads];
    if (status[blockIdx.x] != 0) return;                   // uniform over the block
    const io_png_desc d = desc[blockIdx.x];
    const uint8_t* p = lines + 16 * (long)off[blockIdx.x];
    const long n = png_inflated(d);
    unsigned long long s1 = 0, s2 = 0;
    for (long i = 4L * threadIdx.x; i < n; i += 4L * kThreads) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + i);      // the range is padded to 16 bytes
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) {
                const unsigned long long b = (w >> (8 * k)) & 255u;
                s1 += b;
                s2 += (unsigned long long)(i + k) * b;
            }
    }
    r1[threadIdx.x] = s1 % 65521u;
    r2[threadIdx.x] = s2 % 65521u;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            r1[threadIdx.x] += r1[threadIdx.x + h];
            r2[threadIdx.x] += r2[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && png_adler_finish(r1[0], r2[0], (uint64_t)n) != d.adler) status[blockIdx.x] = PNG_STATUS_ADLER;
}

__device__ __forceinline__ uint32_t png_load_px(const uint8_t* p, int bpp) {
    uint32_t v = 0;
    for (int k = 0; k < bpp; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const io_png_desc* __restrict__ desc,
                                                          const unsigned long long* __restrict__ off, uint8_t* __restrict__ lines,
                                                          int32_t* __restrict__ status) {
    if (status[blockIdx.x] != 0) return;
    const io_png_desc d = desc[blockIdx.x];
    const int bpp = d.channels * (d.depth >> 3);
    const long stride = 1 + png_rowbytes(d);
    uint8_t* base = lines + 16 * (long)off[blockIdx.x];
    const int lane = (int)threadIdx.x;
    int bad = 0;
    for (int y = lane; y < d.H; y += 64) bad |= base[y * stride] > 4;
    if (__syncthreads_or(bad)) {
        if (lane == 0) status[blockIdx.x] = PNG_STATUS_FILTER;
        return;
    }
    for (int y0 = 0; y0 < d.H; y0 += PNG_BAND_ROWS) {
        const int y = y0 + lane;
        const bool live = y < d.H;
        uint8_t* row = base + (live ? y : 0) * stride + 1;
        const int ft = live ? row[-1] : 0;
        uint32_t cur = 0, up_before = 0;                     // this lane's last result; the "above" of the step before
        for (int s = 0; s < d.W + PNG_BAND_ROWS - 1; ++s) {
            const int x = s - lane;
            const bool active = live && x >= 0 && x < d.W;
            uint32_t up = (uint32_t)__shfl_up((int)cur, 1);  // lane r - 1 finished this column one step ago
            if (lane == 0) up = (active && y > 0) ? png_load_px(row - stride + (long)x * bpp, bpp) : 0u;
            if (y == 0) up = 0;
            if (active) {
                const uint32_t left = x > 0 ? cur : 0u, upleft = x > 0 ? up_before : 0u;
                const uint32_t raw = png_load_px(row + (long)x * bpp, bpp);
                uint32_t res = 0;
                for (int k = 0; k < bpp; ++k) {
                    const int a = (left >> (8 * k)) & 255, b = (up >> (8 * k)) & 255, c = (upleft >> (8 * k)) & 255;
                    int pred = 0;
                    if (ft == 1) pred = a;
                    else if (ft == 2) pred = b;
                    else if (ft == 3) pred = (a + b) >> 1;
                    else if (ft == 4) {
                        const int p = a + b - c;
                        const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    }
                    const uint32_t v = (((raw >> (8 * k)) & 255u) + (uint32_t)pred) & 255u;
                    row[(long)x * bpp + k] = (uint8_t)v;
                    res |= v << (8 * k);
                }
                cur = res;
            }
            up_before = up;
        }
        __syncthreads();                                     // the band's last row is in memory for the next band's lane 0
    }
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(const io_png_desc* __restrict__ desc,
                                                            const unsigned long long* __restrict__ off,
                                                            const uint8_t* __restrict__ lines, const int32_t* __restrict__ status,
                                                            uint8_t* __restrict__ out) {
    if (status[blockIdx.y] != 0) return;
    const io_png_desc d = desc[blockIdx.y];
    const long nbytes = png_out_bytes(d);
    uint8_t* dst = out + d.out_off;
    const int head = (int)((uintptr_t)dst & 3);
    const long nwords = (nbytes + head + 3) >> 2;                // aligned words that cover dst[0 .. nbytes)
    if ((long)blockIdx.x * kChunkWords >= nwords) return;
    const uint8_t* src = lines + 16 * (long)off[blockIdx.y];
    const long stride = 1 + png_rowbytes(d);
    const unsigned W = (unsigned)d.W;
#pragma unroll
    for (int jj = 0; jj < kWordsPerThread; ++jj) {
        const long w = (long)blockIdx.x * kChunkWords + jj * kThreads + threadIdx.x;
        if (w >= nwords) break;
        const long p0 = 4 * w - head;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long p = p0 + k;
            if (p < 0 || p >= nbytes) continue;
            unsigned pix, c;                                     // 3 H W < 2^31
            if (d.depth == 16) { pix = (unsigned)p >> 1; c = 1u - ((unsigned)p & 1u); }   // big-endian samples to host order
            else { pix = (unsigned)p / 3u; c = (unsigned)p - 3u * pix; if (d.channels == 1) c = 0; }
            const unsigned y = pix / W, x = pix - y * W;
            const unsigned bpp = (unsigned)d.channels * ((unsigned)d.depth >> 3);
            word |= (unsigned)src[y * stride + 1 + (long)x * bpp + c] << (8 * k);
        }
        if (p0 >= 0 && p0 + 4 <= nbytes) {
            *reinterpret_cast<uint32_t*>(dst + p0) = word;
        } else {                                                 // first / last word of an image: bytes outside it are not ours
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= 0 && p0 + k < nbytes) dst[p0 + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

struct PngPlan {
    size_t off_bytes, line_bytes;
    long max_words;
    double out_bytes;
};

// the checks that need no buffer; *plan filled on success
int png_check_desc(const io_png_desc* desc, int n, PngPlan* plan) {
    IO_REQUIRE(n > 0 && desc, IO_ERR_SHAPE, "png_decode: empty batch or null descriptor table (n=%d)", n);
    IO_REQUIRE(n <= 65535, IO_ERR_SHAPE, "png_decode: n=%d out of range (at most 65535 images per call)", n);
    size_t units = 0;
    long max_words = 0;
    double out_bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const io_png_desc& d = desc[i];
        IO_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535 && 3L * d.H * d.W < (1L << 31), IO_ERR_SHAPE,
                   "png_decode: image %d has size %d x %d (need 1 <= H, W <= 65535 and 3 H W < 2^31)", i, d.H, d.W);
        const bool ok8 = d.depth == 8 && (d.channels == 1 || d.channels == 3 || d.channels == 4);
        IO_REQUIRE(ok8 || (d.depth == 16 && d.channels == 1), IO_ERR_SHAPE,
                   "png_decode: image %d has %d channels of depth %d (1, 3 or 4 of depth 8, or 1 of depth 16)", i, d.channels,
                   d.depth);
        IO_REQUIRE(d.data_off >= 0 && d.data_bytes >= 0, IO_ERR_SHAPE, "png_decode: image %d has a negative data range", i);
        units += (size_t)((png_inflated(d) + 15) >> 4);
        const long words = (png_out_bytes(d) + 3 + 3) / 4;
        if (words > max_words) max_words = words;
        out_bytes += (double)png_out_bytes(d);
    }
    plan->off_bytes = ((size_t)(n + 1) * sizeof(unsigned long long) + 15) / 16 * 16;
    plan->line_bytes = units * 16;
    plan->max_words = max_words;
    plan->out_bytes = out_bytes;
    return IO_OK;
}

}  // namespace

extern "C" int io_png_band_rows(void) { return PNG_BAND_ROWS; }

extern "C" size_t io_png_workspace_bytes(const io_png_desc* desc_host, int n) {
    PngPlan plan;
    if (png_check_desc(desc_host, n, &plan) != IO_OK) return 0;
    return plan.off_bytes + plan.line_bytes;
}

extern "C" int io_png_decode(const uint8_t* pool_dev, size_t pool_bytes, const io_png_desc* desc_dev, const io_png_desc* desc_host,
                             int n, uint8_t* out, size_t out_bytes, void* workspace, size_t workspace_bytes, int32_t* status_dev,
                             hipStream_t st) {
    IO_REQUIRE(pool_dev && desc_dev && out && workspace && status_dev, IO_ERR_SHAPE, "png_decode: null pointer");
    PngPlan plan;
    const int rc = png_check_desc(desc_host, n, &plan);
    if (rc != IO_OK) return rc;
    for (int i = 0; i < n; ++i) {
        const io_png_desc& d = desc_host[i];
        IO_REQUIRE((size_t)d.data_off <= pool_bytes && (size_t)d.data_bytes <= pool_bytes - (size_t)d.data_off, IO_ERR_SHAPE,
                   "png_decode: image %d data outside the byte pool", i);
        const size_t nb = (size_t)png_out_bytes(d);
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && nb <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "png_decode: image %d output outside the output buffer", i);
        IO_REQUIRE(d.depth != 16 || (((uintptr_t)out + (uintptr_t)d.out_off) & 1) == 0, IO_ERR_SHAPE,
                   "png_decode: image %d is 16-bit and its output is not 2-byte aligned", i);
    }
    IO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0, IO_ERR_SHAPE,
               "png_decode: the workspace must be 16-byte aligned, the descriptors 8-byte aligned");
    const size_t need = plan.off_bytes + plan.line_bytes;
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "png_decode: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws);
    uint8_t* lines = ws + plan.off_bytes;
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(64), 0, st, desc_dev, n, off);
    {
        IoProfScope prof(IO_PROF_PNG_INFLATE, 0.0, (double)pool_bytes + 2.0 * (double)plan.line_bytes, st);
        hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, st, pool_dev, desc_dev, off, lines, status_dev);
        hipLaunchKernelGGL(png_adler_kernel, dim3(n), dim3(kThreads), 0, st, desc_dev, off, lines, status_dev);
    }
    {
        IoProfScope prof(IO_PROF_PNG_UNFILTER, 0.0, 2.0 * (double)plan.line_bytes, st);
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64), 0, st, desc_dev, off, lines, status_dev);
    }
    {
        IoProfScope prof(IO_PROF_PNG_PACK, 0.0, (double)plan.line_bytes + plan.out_bytes, st);
        hipLaunchKernelGGL(png_pack_kernel, dim3(io_cdiv(plan.max_words, kChunkWords), n), dim3(kThreads), 0, st, desc_dev, off,
                           lines, status_dev, out);
    }
    return io_check_launch("png_decode");
}

// ---- io_png_decode_par: stage 1 by csrc/png_inflate_par.h ---------------------------------------------------------------------
namespace {

constexpr int kHeadParts = 8;      // workgroups that share the symbols in front of one chunk's tail

// what io_png_decode checks of its buffers, word for word
int png_check_buffers(const io_png_desc* desc_host, int n, size_t pool_bytes, const uint8_t* out, size_t out_bytes,
                      const void* workspace, const io_png_desc* desc_dev) {
    for (int i = 0; i < n; ++i) {
        const io_png_desc& d = desc_host[i];
        IO_REQUIRE((size_t)d.data_off <= pool_bytes && (size_t)d.data_bytes <= pool_bytes - (size_t)d.data_off, IO_ERR_SHAPE,
                   "png_decode: image %d data outside the byte pool", i);
        const size_t nb = (size_t)png_out_bytes(d);
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && nb <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "png_decode: image %d output outside the output buffer", i);
        IO_REQUIRE(d.depth != 16 || (((uintptr_t)out + (uintptr_t)d.out_off) & 1) == 0, IO_ERR_SHAPE,
                   "png_decode: image %d is 16-bit and its output is not 2-byte aligned", i);
    }
    IO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0, IO_ERR_SHAPE,
               "png_decode: the workspace must be 16-byte aligned, the descriptors 8-byte aligned");
    return IO_OK;
}

struct PngParPlan {
    size_t sym_bytes, cb_bytes, flag_bytes, rec_bytes;
    long max_chunks, total_chunks;
};

int png_par_check(const io_png_desc* desc, int n, int chunk_bytes, const PngPlan& plan, PngParPlan* par) {
    IO_REQUIRE(chunk_bytes >= PNG_PAR_MIN_CHUNK && chunk_bytes <= PNG_PAR_MAX_CHUNK && chunk_bytes % PNG_PAR_MIN_CHUNK == 0,
               IO_ERR_SHAPE, "png_decode_par: chunk_bytes=%d (a multiple of %d from %d to %d)", chunk_bytes, PNG_PAR_MIN_CHUNK,
               PNG_PAR_MIN_CHUNK, PNG_PAR_MAX_CHUNK);
    long max_chunks = 0, total = 0;
    for (int i = 0; i < n; ++i) {
        const long c = png_par_chunks(desc[i].data_bytes, chunk_bytes);
        IO_REQUIRE(c <= PNG_PAR_MAX_CHUNKS, IO_ERR_SHAPE, "png_decode_par: image %d has %ld chunks of %d bytes (at most %d)", i, c,
                   chunk_bytes, PNG_PAR_MAX_CHUNKS);
        if (c > max_chunks) max_chunks = c;
        total += c;
    }
    par->sym_bytes = 2 * plan.line_bytes;
    par->cb_bytes = plan.off_bytes;
    par->flag_bytes = png_par_round16(8 * (size_t)n);
    par->rec_bytes = (size_t)PNG_PAR_REC_BYTES * (size_t)total;
    par->max_chunks = max_chunks;
    par->total_chunks = total;
    return IO_OK;
}

// cb[i]: first record of image i
__global__ void png_par_offsets_kernel(const io_png_desc* __restrict__ desc, int n, int chunk_bytes,
                                       unsigned long long* __restrict__ cb) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long at = 0;
    for (int i = 0; i < n; ++i) {
        cb[i] = at;
        at += (unsigned long long)png_par_chunks(desc[i].data_bytes, chunk_bytes);
    }
    cb[n] = at;
}

// a wave per chunk (blockIdx.x) of image blockIdx.y: its candidate, and a record that says "nothing decoded"
__global__ __launch_bounds__(64) void png_par_search_kernel(const uint8_t* __restrict__ pool, const io_png_desc* __restrict__ desc,
                                                            const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                            PngParRec* __restrict__ recs) {
    __shared__ PngShared sh;
    const io_png_desc d = desc[blockIdx.y];
    const long c = blockIdx.x;
    if (c >= png_par_chunks(d.data_bytes, chunk_bytes)) return;
    long cand = 0;
    if (c > 0) {
        const long lo = 8L * c * chunk_bytes, end = 8L * d.data_bytes;
        const long hi = lo + 8L * chunk_bytes < end ? lo + 8L * chunk_bytes : end;
        cand = png_par_search(&sh, pool + d.data_off, d.data_bytes, lo, hi, (int)threadIdx.x, 64);
    }
    if (threadIdx.x == 0) {
        PngParRec& r = recs[cb[blockIdx.y] + c];
        r.cand = cand; r.exit_bit = 0; r.n = 0; r.offset = -1;
        r.reach = 0; r.exit = PNG_EXIT_NONE; r.status = 0; r.next = -1;
    }
}

__global__ __launch_bounds__(64) void png_par_count_kernel(const uint8_t* __restrict__ pool, const io_png_desc* __restrict__ desc,
                                                           const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                           PngParRec* __restrict__ recs) {
    __shared__ PngShared sh;
    const io_png_desc d = desc[blockIdx.y];
    const long c = blockIdx.x;
    const int nchunks = (int)png_par_chunks(d.data_bytes, chunk_bytes);
    if (c >= nchunks) return;
    PngParRec* mine = recs + cb[blockIdx.y];
    const long cand = (long)mine[c].cand;                    // uniform over the wave
    if (cand < 0) return;
    PngParOut r;
    png_par_decode<false>(&sh, nullptr, pool + d.data_off, d.data_bytes, cand, png_inflated(d), mine, nchunks, chunk_bytes,
                          nullptr, 0, r, (int)threadIdx.x, 64);
    if (threadIdx.x == 0) {
        PngParRec& o = mine[c];
        o.exit_bit = r.exit_bit; o.n = r.n; o.reach = r.reach; o.exit = r.exit; o.status = r.status; o.next = r.next;
    }
}

// a lane per image: offsets along the chain, the info word, the two predicates, status 0 for an image stored in parallel
__global__ __launch_bounds__(kThreads) void png_par_chain_kernel(const io_png_desc* __restrict__ desc, int n,
                                                                 const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                                 PngParRec* __restrict__ recs, int32_t* __restrict__ flags,
                                                                 int32_t* __restrict__ info, int32_t* __restrict__ status) {
    const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    const io_png_desc d = desc[i];
    const int word = png_par_chain(recs + cb[i], (int)png_par_chunks(d.data_bytes, chunk_bytes), png_inflated(d));
    const int par = (word >> 16) == 0;
    flags[2 * i] = par;
    flags[2 * i + 1] = !par;
    if (info) info[i] = word;
    if (par) status[i] = 0;
}

// a wave per chain chunk of an image stored in parallel: the symbols.  68.8 KiB of LDS: two chunks per CU.
__global__ __launch_bounds__(64) void png_par_store_kernel(const uint8_t* __restrict__ pool, const io_png_desc* __restrict__ desc,
                                                           const unsigned long long* __restrict__ off,
                                                           const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                           const PngParRec* __restrict__ recs, uint16_t* __restrict__ syms,
                                                           int32_t* __restrict__ flags) {
    __shared__ PngShared sh;
    __shared__ uint8_t hi[PNG_RING_BYTES];
    const long c = blockIdx.x;
    const io_png_desc d = desc[blockIdx.y];
    const int nchunks = (int)png_par_chunks(d.data_bytes, chunk_bytes);
    if (c >= nchunks || !flags[2 * blockIdx.y]) return;      // not stored in parallel
    const PngParRec* mine = recs + cb[blockIdx.y];
    const PngParRec rec = mine[c];
    const long expected = png_inflated(d);
    if (rec.offset < 0 || rec.offset + rec.n > expected) return;     // not on the chain (the second test never fails: the chain checked it)
    PngParOut r;
    png_par_decode<true>(&sh, hi, pool + d.data_off, d.data_bytes, (long)rec.cand, expected, mine, nchunks, chunk_bytes,
                         syms + 16 * (long)off[blockIdx.y] + rec.offset, (long)rec.n, r, (int)threadIdx.x, 64);
    if (threadIdx.x == 0 && (r.exit != rec.exit || r.exit_bit != rec.exit_bit || r.n != rec.n || r.reach != rec.reach))
        flags[2 * blockIdx.y + 1] = 2;                    // the pass disagrees with its record: the sequential kernel decodes
}

__global__ __launch_bounds__(kThreads) void png_par_tail_kernel(const io_png_desc* __restrict__ desc,
                                                                const unsigned long long* __restrict__ off,
                                                                const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                                const PngParRec* __restrict__ recs, const uint16_t* __restrict__ syms,
                                                                uint8_t* __restrict__ lines, const int32_t* __restrict__ flags) {
    const int i = blockIdx.x;
    if (!flags[2 * i] || flags[2 * i + 1]) return;           // uniform over the block
    const io_png_desc d = desc[i];
    png_par_tail(recs + cb[i], (int)png_par_chunks(d.data_bytes, chunk_bytes), png_inflated(d), syms + 16 * (long)off[i],
                 lines + 16 * (long)off[i], (int)threadIdx.x, kThreads);
}

__global__ __launch_bounds__(kThreads) void png_par_head_kernel(const io_png_desc* __restrict__ desc,
                                                                const unsigned long long* __restrict__ off,
                                                                const unsigned long long* __restrict__ cb, int chunk_bytes,
                                                                const PngParRec* __restrict__ recs, const uint16_t* __restrict__ syms,
                                                                uint8_t* __restrict__ lines, const int32_t* __restrict__ flags) {
    const int i = blockIdx.y;
    const long c = blockIdx.x;
    if (!flags[2 * i] || flags[2 * i + 1]) return;
    const io_png_desc d = desc[i];
    if (c >= png_par_chunks(d.data_bytes, chunk_bytes)) return;
    const PngParRec rec = recs[cb[i] + c];
    if (rec.offset < 0 || rec.offset + rec.n > png_inflated(d)) return;
    png_par_head(rec, syms + 16 * (long)off[i], lines + 16 * (long)off[i], (long)blockIdx.z * kThreads + threadIdx.x,
                 (long)kHeadParts * kThreads);
}

// png_inflate_kernel under a per-image predicate: flags[2 i + 1] says that the sequential decoder takes image i
__global__ __launch_bounds__(64) void png_inflate_pred_kernel(const uint8_t* __restrict__ pool, const io_png_desc* __restrict__ desc,
                                                              const unsigned long long* __restrict__ off, uint8_t* __restrict__ lines,
                                                              int32_t* __restrict__ status, const int32_t* __restrict__ flags) {
    __shared__ PngShared sh;
    if (!flags[2 * blockIdx.x + 1]) return;                  // uniform over the wave
    const io_png_desc d = desc[blockIdx.x];
    const int rc = png_inflate(&sh, pool + d.data_off, d.data_bytes, lines + 16 * (long)off[blockIdx.x], png_inflated(d),
                               (int)threadIdx.x, 64);
    if (threadIdx.x == 0) status[blockIdx.x] = rc;
}

}  // namespace

extern "C" size_t io_png_par_workspace_bytes(const io_png_desc* desc_host, int n, int chunk_bytes) {
    PngPlan plan;
    PngParPlan par;
    if (png_check_desc(desc_host, n, &plan) != IO_OK || png_par_check(desc_host, n, chunk_bytes, plan, &par) != IO_OK) return 0;
    return plan.off_bytes + plan.line_bytes + par.sym_bytes + par.cb_bytes + par.flag_bytes + par.rec_bytes;
}

extern "C" int io_png_decode_par(const uint8_t* pool_dev, size_t pool_bytes, const io_png_desc* desc_dev,
                                 const io_png_desc* desc_host, int n, uint8_t* out, size_t out_bytes, void* workspace,
                                 size_t workspace_bytes, int32_t* status_dev, int chunk_bytes, int32_t* info_dev, hipStream_t st) {
    IO_REQUIRE(pool_dev && desc_dev && out && workspace && status_dev, IO_ERR_SHAPE, "png_decode_par: null pointer");
    PngPlan plan;
    int rc = png_check_desc(desc_host, n, &plan);
    if (rc != IO_OK) return rc;
    rc = png_check_buffers(desc_host, n, pool_bytes, out, out_bytes, workspace, desc_dev);
    if (rc != IO_OK) return rc;
    PngParPlan par;
    rc = png_par_check(desc_host, n, chunk_bytes, plan, &par);
    if (rc != IO_OK) return rc;
    const size_t need = plan.off_bytes + plan.line_bytes + par.sym_bytes + par.cb_bytes + par.flag_bytes + par.rec_bytes;
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "png_decode_par: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws);
    uint8_t* lines = ws + plan.off_bytes;
    uint16_t* syms = reinterpret_cast<uint16_t*>(lines + plan.line_bytes);
    unsigned long long* cb = reinterpret_cast<unsigned long long*>(lines + plan.line_bytes + par.sym_bytes);
    int32_t* flags = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(cb) + par.cb_bytes);
    PngParRec* recs = reinterpret_cast<PngParRec*>(reinterpret_cast<uint8_t*>(flags) + par.flag_bytes);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(64), 0, st, desc_dev, n, off);
    hipLaunchKernelGGL(png_par_offsets_kernel, dim3(1), dim3(64), 0, st, desc_dev, n, chunk_bytes, cb);
    const dim3 per_chunk((unsigned)(par.max_chunks > 0 ? par.max_chunks : 1), (unsigned)n);
    {
        IoProfScope prof(IO_PROF_PNG_PAR_SEARCH, 0.0, (double)pool_bytes, st);
        hipLaunchKernelGGL(png_par_search_kernel, per_chunk, dim3(64), 0, st, pool_dev, desc_dev, cb, chunk_bytes, recs);
    }
    {
        IoProfScope prof(IO_PROF_PNG_PAR_COUNT, 0.0, (double)pool_bytes, st);
        hipLaunchKernelGGL(png_par_count_kernel, per_chunk, dim3(64), 0, st, pool_dev, desc_dev, cb, chunk_bytes, recs);
        hipLaunchKernelGGL(png_par_chain_kernel, dim3(io_cdiv(n, kThreads)), dim3(kThreads), 0, st, desc_dev, n, cb, chunk_bytes,
                           recs, flags, info_dev, status_dev);
    }
    {
        IoProfScope prof(IO_PROF_PNG_PAR_STORE, 0.0, (double)pool_bytes + (double)par.sym_bytes, st);
        hipLaunchKernelGGL(png_par_store_kernel, per_chunk, dim3(64), 0, st, pool_dev, desc_dev, off, cb, chunk_bytes, recs, syms,
                           flags);
    }
    {
        IoProfScope prof(IO_PROF_PNG_PAR_RESOLVE, 0.0, (double)par.sym_bytes + (double)plan.line_bytes, st);
        hipLaunchKernelGGL(png_par_tail_kernel, dim3(n), dim3(kThreads), 0, st, desc_dev, off, cb, chunk_bytes, recs, syms, lines,
                           flags);
        hipLaunchKernelGGL(png_par_head_kernel, dim3(per_chunk.x, per_chunk.y, kHeadParts), dim3(kThreads), 0, st, desc_dev, off, cb,
                           chunk_bytes, recs, syms, lines, flags);
    }
    {
        IoProfScope prof(IO_PROF_PNG_INFLATE, 0.0, (double)pool_bytes + 2.0 * (double)plan.line_bytes, st);
        hipLaunchKernelGGL(png_inflate_pred_kernel, dim3(n), dim3(64), 0, st, pool_dev, desc_dev, off, lines, status_dev, flags);
        hipLaunchKernelGGL(png_adler_kernel, dim3(n), dim3(kThreads), 0, st, desc_dev, off, lines, status_dev);
    }
    {
        IoProfScope prof(IO_PROF_PNG_UNFILTER, 0.0, 2.0 * (double)plan.line_bytes, st);
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64), 0, st, desc_dev, off, lines, status_dev);
    }
    {
        IoProfScope prof(IO_PROF_PNG_PACK, 0.0, (double)plan.line_bytes + plan.out_bytes, st);
        hipLaunchKernelGGL(png_pack_kernel, dim3(io_cdiv(plan.max_words, kChunkWords), n), dim3(kThreads), 0, st, desc_dev, off,
                           lines, status_dev, out);
    }
    return io_check_launch("png_decode_par");
}
