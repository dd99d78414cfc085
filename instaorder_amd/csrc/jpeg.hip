// Baseline JPEG files -> interleaved uint8 RGB images, on the device (DESIGN.md "JPEG images").
//
// The headers are parsed by the caller; per image the entropy-coded bytes, a table set and a descriptor arrive
// (include/instaorder_hip.h).  The result is the published baseline algorithm with libjpeg's default choices, integer only:
//   0. jpeg_offsets_kernel   exclusive prefix sum of the images' 8 x 8 block counts: where an image's coefficients (128 B
//      jpeg_tables_kernel    per block) and planes (64 B per block) start; the derived Huffman tables of every table set.
//   1. jpeg_entropy_kernel   the sequential part (jpeg_entropy.h): ONE LANE PER IMAGE, io_jpeg_set_images_per_wave() lanes (default 1)
//                            of a wave64 in use; the bytes are read eight at a time, the derived tables from LDS when the
//                            batch has at most IO_JPEG_LDS_TABLE_SETS sets, else from global memory.  Writes the non-zero quantised
//                            coefficients as int16 into the zeroed coefficient range and a status word per image.
//   2. jpeg_idct_kernel      one thread per block: dequantise, the "islow" IDCT of jidctint.c (13-bit constants, columns
//                            descaled by 11, rows by 18, + 128, clamp), 8 x 8 bytes into the component plane, which is
//                            padded to whole MCUs.
//   3. jpeg_colour_kernel    as rle_decode_kernel: a thread owns one aligned 4-byte word of the output, computes the (at
//                            most two) pixels its bytes belong to -- triangle upsampling of the chroma planes over their
//                            REAL width and height, 16-bit fixed-point YCbCr -> RGB -- and stores the word once.
//   1p. jpeg_sync_kernel     (io_jpeg_decode_par_u8 only) stage 1 on MANY lanes per image: one 256-thread block per image runs the
//      jpeg_fallback_kernel  self-synchronising scheme of jpeg_sync.h -- threads stride over the subsequences of the scan, the
//                            rounds loop inside the kernel -- and stores the coefficients of a clean image; every other
//                            image is decoded by the one-lane loop of stage 1, launched behind it with a per-image predicate.
//   1g. jpeg_prog_entropy_kernel (io_jpeg_decode_prog_u8 only) stage 1 of PROGRESSIVE files (jpeg_prog.h): one 256-thread block per
//                            image fills the coefficient range over the file's scans, level by level with a block barrier
//                            between levels, the scans of a level on one lane each of different waves.
// All arithmetic is 32-bit two's complement, which holds every intermediate of a stream an encoder made from 8-bit samples.
//
// Safety does not depend on the pool or table bytes: see jpeg_entropy.h for stage 1; stages 2 and 3 read and write only
// addresses that follow from the descriptors the host validated, and every sample is clamped to a byte before it is stored.
#include "io_common.h"
#include "jpeg_entropy.h"
#include "jpeg_prog.h"
#include "jpeg_sync.h"

#include <atomic>
#include <vector>

namespace {

constexpr int kThreads = 256;                // four wave64
constexpr int kWordsPerThread = 4;           // colour: 16 output bytes per thread and chunk
constexpr int kChunkWords = kThreads * kWordsPerThread;
static_assert(sizeof(io_jpeg_tables) == 1600 && sizeof(io_jpeg_desc) == 64, "ABI layout of the JPEG tables");
static_assert(sizeof(JpegHuff) == 904, "four derived tables per set keep 16-byte alignment");

// images per wave64 of the entropy stage.  Measured on 256 noise images of 640 x 480 (tools/jpeg_input_bench.py): 1 was the
// fastest of 64 / 16 / 4 / 1 -- the lanes of a wave diverge on every symbol and each waits for the others' memory reads
std::atomic<int> g_images_per_wave{1};

struct Geo {
    int mw, mh;          // MCUs across and down
    int bpm;             // blocks per MCU
    long n_blocks;
    int ystride, cstride;// bytes per row of the padded luma / chroma plane
    long ybytes, cbytes; // bytes of the padded luma plane / of one chroma plane
};

__host__ __device__ inline Geo geometry(const io_jpeg_desc& d) {
    Geo g;
    g.mw = (d.W + 8 * d.hs - 1) / (8 * d.hs);
    g.mh = (d.H + 8 * d.vs - 1) / (8 * d.vs);
    g.bpm = d.hs * d.vs + (d.n_comp == 3 ? 2 : 0);
    g.n_blocks = (long)g.mw * g.mh * g.bpm;
    g.ystride = g.mw * 8 * d.hs;
    g.cstride = g.mw * 8;
    g.ybytes = (long)g.ystride * (g.mh * 8 * d.vs);
    g.cbytes = d.n_comp == 3 ? (long)g.cstride * (g.mh * 8) : 0;
    return g;
}

// off[i] = blocks of the images before i, off[n] = all blocks (one block of threads)
__global__ __launch_bounds__(kThreads) void jpeg_offsets_kernel(const io_jpeg_desc* __restrict__ desc, int n,
                                                                unsigned long long* __restrict__ off) {
    __shared__ unsigned long long s[kThreads];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += kThreads) {             // block-uniform trip count
        const int i = base + tid;
        const unsigned long long w = i < n ? (unsigned long long)geometry(desc[i]).n_blocks : 0ull;
        s[tid] = w;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {
            const unsigned long long v = tid >= d ? s[tid - d] : 0ull;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        if (i < n) off[i] = carry + s[tid] - w;
        carry += s[kThreads - 1];
        __syncthreads();
    }
    if (tid == 0) off[n] = carry;
}

__global__ __launch_bounds__(64) void jpeg_tables_kernel(const io_jpeg_tables* __restrict__ tables, JpegHuff* __restrict__ huff) {
    if (threadIdx.x >= 4) return;
    const io_jpeg_tables& t = tables[blockIdx.x];
    (void)jpeg_build_huff(t.huff_counts[threadIdx.x], t.huff_symbols[threadIdx.x], huff + 4 * blockIdx.x + threadIdx.x);
}

// the scan of image d with the derived tables at `set` (LDS or global: one copy of the loop per address space)
__device__ __forceinline__ int decode_image(const io_jpeg_desc& d, const uint8_t* __restrict__ pool, const JpegHuff* set,
                                            int16_t* __restrict__ coef) {
    const Geo g = geometry(d);
    JpegScan s;
    s.data = pool + d.data_off;
    s.nbytes = d.data_bytes;
    s.n_mcu = g.mw * g.mh;
    s.luma_blocks = d.hs * d.vs;
    s.chroma = d.n_comp == 3 ? 1 : 0;
    s.restart_interval = d.restart_interval;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.dc[c] = set + (d.dc[c] & 1);
        s.ac[c] = set + 2 + (d.ac[c] & 1);
    }
    return jpeg_decode_scan(s, coef);
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(const uint8_t* __restrict__ pool,
                                                                const JpegHuff* __restrict__ huff, int n_sets,
                                                                const io_jpeg_desc* __restrict__ desc,
                                                                const unsigned long long* __restrict__ off,
                                                                int16_t* __restrict__ coef, int32_t* __restrict__ status,
                                                                int n, int per_wave) {
    // the derived tables of a batch with at most IO_JPEG_LDS_TABLE_SETS table sets are staged in LDS: a lookup is then an
    // LDS read, which does not wait for the coefficient stores in flight as a global read does
    __shared__ uint32_t s_huff[IO_JPEG_LDS_TABLE_SETS * 4 * sizeof(JpegHuff) / 4];
    const bool staged = n_sets <= IO_JPEG_LDS_TABLE_SETS;        // block-uniform
    if (staged) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff);
        const int words = n_sets * 4 * (int)(sizeof(JpegHuff) / 4);
        for (int k = threadIdx.x; k < words; k += kThreads) s_huff[k] = src[k];
        __syncthreads();
    }
    const int wave = (int)((blockIdx.x * (unsigned)kThreads + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (lane >= per_wave) return;
    const long i = (long)wave * per_wave + lane;
    if (i >= n) return;
    const io_jpeg_desc d = desc[i];
    int16_t* dst = coef + 64 * (long)off[i];
    int st;
    if (staged) st = decode_image(d, pool, reinterpret_cast<const JpegHuff*>(s_huff) + 4 * (long)d.table_set, dst);
    else st = decode_image(d, pool, huff + 4 * (long)d.table_set, dst);
    status[i] = st;
}

// ---- stage 1 on many lanes (jpeg_sync.h) --------------------------------------------------------------------------------
// suboff[i] = subsequences of the images before i, suboff[n] = all of them (one block of threads)
__global__ __launch_bounds__(kThreads) void jpeg_sub_offsets_kernel(const io_jpeg_desc* __restrict__ desc, int n, int subseq_bytes,
                                                                    unsigned long long* __restrict__ suboff) {
    __shared__ unsigned long long s[kThreads];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += kThreads) {             // block-uniform trip count
        const int i = base + tid;
        const unsigned long long w = i < n ? (unsigned long long)jpeg_sync_count(desc[i].data_bytes, subseq_bytes) : 0ull;
        s[tid] = w;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {
            const unsigned long long v = tid >= d ? s[tid - d] : 0ull;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        if (i < n) suboff[i] = carry + s[tid] - w;
        carry += s[kThreads - 1];
        __syncthreads();
    }
    if (tid == 0) suboff[n] = carry;
}

// One block per image; thread t owns the subsequences t, t + 256, ...  Every barrier is reached by all threads: the trip
// counts of the strided loops differ per thread, the barriers stand outside them, and the rounds loop ends on a flag in LDS
// that all threads read behind a barrier.  The records live in the workspace (64 bytes per subsequence, word-major).
__global__ __launch_bounds__(kThreads) void jpeg_sync_kernel(const uint8_t* __restrict__ pool, const JpegHuff* __restrict__ huff,
                                                             const io_jpeg_desc* __restrict__ desc,
                                                             const unsigned long long* __restrict__ off,
                                                             const unsigned long long* __restrict__ suboff,
                                                             uint32_t* __restrict__ rec_all, int16_t* __restrict__ coef,
                                                             int32_t* __restrict__ status, int32_t* __restrict__ fallback,
                                                             int32_t* __restrict__ info, int subseq_bytes, int max_rounds) {
    __shared__ uint32_t s_huff[4 * sizeof(JpegHuff) / 4];
    __shared__ int s_changed[2];
    __shared__ int s_live;
    const int img = blockIdx.x, tid = threadIdx.x;
    const io_jpeg_desc d = desc[img];
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + 4 * (long)d.table_set);
        for (int k = tid; k < 4 * (int)(sizeof(JpegHuff) / 4); k += kThreads) s_huff[k] = src[k];
        if (tid < 2) s_changed[tid] = 0;
    }
    const Geo g = geometry(d);
    const JpegHuff* set = reinterpret_cast<const JpegHuff*>(s_huff);
    JpegScan s;
    s.data = pool + d.data_off;
    s.nbytes = d.data_bytes;
    s.n_mcu = g.mw * g.mh;
    s.luma_blocks = d.hs * d.vs;
    s.chroma = d.n_comp == 3 ? 1 : 0;
    s.restart_interval = d.restart_interval;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s.dc[c] = set + (d.dc[c] & 1);
        s.ac[c] = set + 2 + (d.ac[c] & 1);
    }
    const int32_t nsub = jpeg_sync_count(d.data_bytes, subseq_bytes);
    uint32_t* rec = rec_all + (size_t)JS_WORDS * suboff[img];
    for (int32_t i = tid; i < nsub; i += kThreads) jpeg_sync_init_one(s, rec, nsub, i, subseq_bytes);
    __syncthreads();
    int rounds = 0;
    bool converged = false;
    for (int t = 1; t <= max_rounds; ++t) {                      // block-uniform: ends on s_changed, read behind a barrier
        for (int32_t i = tid; i < nsub; i += kThreads) jpeg_sync_round_one(s, rec, nsub, i, subseq_bytes);
        __syncthreads();
        if (tid == 0) s_changed[(t + 1) & 1] = 0;                // last read before the barrier above, next written behind the one below
        bool any = false;
        for (int32_t i = tid; i < nsub; i += kThreads) any = jpeg_sync_entry_one(rec, nsub, i) || any;
        if (any) atomicOr(&s_changed[t & 1], 1);
        __syncthreads();
        rounds = t;
        if (!s_changed[t & 1]) {
            converged = true;
            break;
        }
    }
    if (tid == 0) {
        const int32_t live = converged ? jpeg_sync_finish(rec, nsub, g.n_blocks) : 0;
        const int32_t word = rounds | (!converged ? JPEG_INFO_NOT_CONVERGED : (live == 0 ? JPEG_INFO_NOT_CLEAN : 0));
        s_live = live;
        fallback[img] = word >> 16;
        if (info) info[img] = word;
        if (live) status[img] = JPEG_STATUS_OK;
    }
    __syncthreads();
    const int32_t live = s_live;
    int16_t* dst = coef + 64 * (long)off[img];
    for (int32_t i = tid; i < live; i += kThreads) jpeg_sync_write_one(s, rec, nsub, i, subseq_bytes, dst, g.n_blocks);
}

// jpeg_entropy_kernel with one image per wave, for the images jpeg_sync_kernel left: fallback[i] != 0
__global__ __launch_bounds__(kThreads) void jpeg_fallback_kernel(const uint8_t* __restrict__ pool, const JpegHuff* __restrict__ huff,
                                                                 int n_sets, const io_jpeg_desc* __restrict__ desc,
                                                                 const unsigned long long* __restrict__ off,
                                                                 int16_t* __restrict__ coef, int32_t* __restrict__ status,
                                                                 const int32_t* __restrict__ fallback, int n) {
    __shared__ uint32_t s_huff[IO_JPEG_LDS_TABLE_SETS * 4 * sizeof(JpegHuff) / 4];
    constexpr int kWaves = kThreads / 64;
    bool need = false;                                           // block-uniform: the block's images, read by every thread
    for (int w = 0; w < kWaves; ++w) {
        const long j = (long)blockIdx.x * kWaves + w;
        if (j < n && fallback[j]) need = true;
    }
    if (!need) return;
    const bool staged = n_sets <= IO_JPEG_LDS_TABLE_SETS;
    if (staged) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff);
        const int words = n_sets * 4 * (int)(sizeof(JpegHuff) / 4);
        for (int k = threadIdx.x; k < words; k += kThreads) s_huff[k] = src[k];
        __syncthreads();
    }
    const long i = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) != 0 || i >= n || !fallback[i]) return;
    const io_jpeg_desc d = desc[i];
    int16_t* dst = coef + 64 * (long)off[i];
    int st;
    if (staged) st = decode_image(d, pool, reinterpret_cast<const JpegHuff*>(s_huff) + 4 * (long)d.table_set, dst);
    else st = decode_image(d, pool, huff + 4 * (long)d.table_set, dst);
    status[i] = st;
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------------
constexpr int kNatOfZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct ZigOfNat {
    int v[64];
    constexpr ZigOfNat() : v() {
        for (int k = 0; k < 64; ++k) v[kNatOfZig[k]] = k;
    }
};
constexpr ZigOfNat kZigOfNat;

// one 8-point pass of jidctint.c (CONST_BITS 13), without the descale
__device__ __forceinline__ void idct8(const int* in, int stride, int* o) {
    const int i0 = in[0], i1 = in[stride], i2 = in[2 * stride], i3 = in[3 * stride], i4 = in[4 * stride],
              i5 = in[5 * stride], i6 = in[6 * stride], i7 = in[7 * stride];
    int z1 = (i2 + i6) * 4433;
    const int t2 = z1 + i6 * (-15137), t3 = z1 + i2 * 6270;
    const int t0 = (i0 + i4) * 8192, t1 = (i0 - i4) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446;
    a1 *= 16819;
    a2 *= 25172;
    a3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    o[0] = t10 + a3;
    o[1] = t11 + a2;
    o[2] = t12 + a1;
    o[3] = t13 + a0;
    o[4] = t13 - a0;
    o[5] = t12 - a1;
    o[6] = t11 - a2;
    o[7] = t10 - a3;
}

__device__ __forceinline__ unsigned clamp_byte(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const io_jpeg_tables* __restrict__ tables,
                                                             const io_jpeg_desc* __restrict__ desc,
                                                             const unsigned long long* __restrict__ off,
                                                             const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                             int n) {
    const unsigned long long b = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (b >= off[n]) return;
    int lo = 0, hi = n;                                          // the image with off[i] <= b < off[i + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= b) lo = mid;
        else hi = mid;
    }
    const io_jpeg_desc d = desc[lo];
    const Geo g = geometry(d);
    const long j = (long)(b - off[lo]);                          // block of the image in decode order
    const int mcu = (int)(j / g.bpm), r = (int)(j - (long)mcu * g.bpm);
    const int my = mcu / g.mw, mx = mcu - my * g.mw;
    const int luma = d.hs * d.vs;
    int comp, brow, bcol, stride;
    uint8_t* plane = planes + 64 * (long)off[lo];
    if (r < luma) {
        comp = 0;
        brow = my * d.vs + r / d.hs;
        bcol = mx * d.hs + r % d.hs;
        stride = g.ystride;
    } else {
        comp = 1 + (r - luma);
        brow = my;
        bcol = mx;
        stride = g.cstride;
        plane += g.ybytes + (comp - 1) * g.cbytes;
    }
    const uint16_t* q = tables[d.table_set].quant[d.quant[comp] & 3];
    const int16_t* c = coef + 64 * (long)b;
    int v[64], ws[64], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                // a row of 8 coefficients and 8 table entries per load
        const uint4 cw = *reinterpret_cast<const uint4*>(c + 8 * k);
        const uint4 qw = *reinterpret_cast<const uint4*>(q + 8 * k);
        const unsigned cc[4] = {cw.x, cw.y, cw.z, cw.w}, qq[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[8 * k + 2 * e] = (int)(int16_t)(cc[e] & 0xffffu);
            v[8 * k + 2 * e + 1] = (int)(int16_t)(cc[e] >> 16);
            ws[8 * k + 2 * e] = (int)(qq[e] & 0xffffu);           // ws holds the table (zig-zag order) until the first pass
            ws[8 * k + 2 * e + 1] = (int)(qq[e] >> 16);
        }
    }
#pragma unroll
    for (int p = 0; p < 64; ++p) v[p] *= ws[kZigOfNat.v[p]];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        idct8(v + x, 8, o);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[8 * y + x] = (o[y] + (1 << 10)) >> 11;
    }
    uint8_t* dst = plane + (long)brow * 8 * stride + bcol * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        idct8(ws + 8 * y, 1, o);
        unsigned w0 = 0, w1 = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            w0 |= clamp_byte(((o[x] + (1 << 17)) >> 18) + 128) << (8 * x);
            w1 |= clamp_byte(((o[x + 4] + (1 << 17)) >> 18) + 128) << (8 * x);
        }
        uint32_t* row = reinterpret_cast<uint32_t*>(dst + (long)y * stride);   // plane rows are multiples of 8 bytes
        row[0] = w0;
        row[1] = w1;
    }
}

// ---- stage 3 -----------------------------------------------------------------------------------------------------------
// the chroma sample of output pixel (y, x): triangle filter over the cw x ch REAL samples of the plane
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int y,
                                         int x) {
    if (hs == 1) return p[(long)y * stride + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(long)(vs == 2 ? y >> 1 : y) * stride + cx];    // libjpeg filters only planes wider than two samples
    const int ox = (x & 1) ? (cx + 1 < cw ? cx + 1 : cw - 1) : (cx > 0 ? cx - 1 : 0);
    if (vs == 1) {
        const uint8_t* row = p + (long)y * stride;
        return (3 * row[cx] + row[ox] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    const int fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* near = p + (long)cy * stride;
    const uint8_t* far = p + (long)fy * stride;
    const int t = 3 * near[cx] + far[cx], to = 3 * near[ox] + far[ox];
    return (3 * t + to + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(const io_jpeg_desc* __restrict__ desc,
                                                               const unsigned long long* __restrict__ off,
                                                               const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
    const io_jpeg_desc d = desc[blockIdx.y];
    const long nbytes = 3L * d.H * d.W;
    uint8_t* dst = out + d.out_off;
    const int head = (int)((uintptr_t)dst & 3);
    const long nwords = (nbytes + head + 3) >> 2;                // aligned words that cover dst[0 .. nbytes)
    if ((long)blockIdx.x * kChunkWords >= nwords) return;
    const Geo g = geometry(d);
    const uint8_t* yp = planes + 64 * (long)off[blockIdx.y];
    const uint8_t* cbp = yp + g.ybytes;
    const uint8_t* crp = cbp + g.cbytes;
    const int cw = (d.W + d.hs - 1) / d.hs, ch = (d.H + d.vs - 1) / d.vs;
#pragma unroll
    for (int jj = 0; jj < kWordsPerThread; ++jj) {
        const long w = (long)blockIdx.x * kChunkWords + jj * kThreads + threadIdx.x;
        if (w >= nwords) break;
        const long p0 = 4 * w - head;
        unsigned word = 0;
        long have = -1;                                          // the pixel whose colour is in rgb
        unsigned rgb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long p = p0 + k;
            if (p < 0 || p >= nbytes) continue;
            const unsigned pix = (unsigned)p / 3u, c = (unsigned)p - 3u * pix;     // 3 H W < 2^31
            if ((long)pix != have) {
                have = pix;
                const int y = (int)(pix / (unsigned)d.W), x = (int)(pix - (unsigned)y * (unsigned)d.W);
                const int Y = yp[(long)y * g.ystride + x];
                if (d.n_comp == 3) {
                    const int cb = chroma_at(cbp, g.cstride, cw, ch, d.hs, d.vs, y, x) - 128;
                    const int cr = chroma_at(crp, g.cstride, cw, ch, d.hs, d.vs, y, x) - 128;
                    const unsigned R = clamp_byte(Y + ((91881 * cr + 32768) >> 16));
                    const unsigned G = clamp_byte(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    const unsigned B = clamp_byte(Y + ((116130 * cb + 32768) >> 16));
                    rgb = R | (G << 8) | (B << 16);
                } else {
                    rgb = (unsigned)Y * 0x010101u;
                }
            }
            word |= ((rgb >> (8 * c)) & 0xffu) << (8 * k);
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

struct JpegPlan {
    long total_blocks, max_words;
    int n_sets;
    size_t off_bytes, huff_bytes, coef_bytes, plane_bytes;
    double out_bytes;
};

// the checks that need no buffer; *plan filled on success
int jpeg_check_desc(const io_jpeg_desc* desc, int n, JpegPlan* plan) {
    IO_REQUIRE(n > 0 && desc, IO_ERR_SHAPE, "jpeg_decode: empty batch or null descriptor table (n=%d)", n);
    IO_REQUIRE(n <= 65535, IO_ERR_SHAPE, "jpeg_decode: n=%d out of range (at most 65535 images per call)", n);
    long blocks = 0, max_words = 0;
    int n_sets = 0;
    double out_bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const io_jpeg_desc& d = desc[i];
        IO_REQUIRE(d.H >= 1 && d.W >= 1 && d.H <= 65535 && d.W <= 65535 && 3L * d.H * d.W < (1L << 31), IO_ERR_SHAPE,
                   "jpeg_decode: image %d has size %d x %d (need 1 <= H, W <= 65535 and 3 H W < 2^31)", i, d.H, d.W);
        const bool gray = d.n_comp == 1 && d.hs == 1 && d.vs == 1;
        const bool ycc = d.n_comp == 3 && ((d.hs == 1 && d.vs == 1) || (d.hs == 2 && (d.vs == 1 || d.vs == 2)));
        IO_REQUIRE(gray || ycc, IO_ERR_SHAPE,
                   "jpeg_decode: image %d has %d components with luma sampling %d x %d (1 with 1x1, or 3 with 1x1, 2x1, 2x2)", i,
                   d.n_comp, d.hs, d.vs);
        IO_REQUIRE(d.restart_interval >= 0, IO_ERR_SHAPE, "jpeg_decode: image %d has restart_interval=%d", i,
                   d.restart_interval);
        IO_REQUIRE(d.table_set >= 0 && d.table_set <= 65535, IO_ERR_SHAPE, "jpeg_decode: image %d names table set %d", i,
                   d.table_set);
        for (int c = 0; c < d.n_comp; ++c)
            IO_REQUIRE(d.quant[c] < 4 && d.dc[c] < 2 && d.ac[c] < 2, IO_ERR_SHAPE,
                       "jpeg_decode: image %d component %d names tables quant=%d dc=%d ac=%d (quant < 4, Huffman < 2)", i, c,
                       d.quant[c], d.dc[c], d.ac[c]);
        IO_REQUIRE(d.data_off >= 0 && d.data_bytes >= 0, IO_ERR_SHAPE, "jpeg_decode: image %d has a negative data range", i);
        if (d.table_set + 1 > n_sets) n_sets = d.table_set + 1;
        blocks += geometry(d).n_blocks;
        IO_REQUIRE(blocks < (1L << 31), IO_ERR_SHAPE, "jpeg_decode: more than 2^31 blocks in one call");
        const long words = (3L * d.H * d.W + 3 + 3) / 4;
        if (words > max_words) max_words = words;
        out_bytes += 3.0 * d.H * d.W;
    }
    plan->total_blocks = blocks;
    plan->max_words = max_words;
    plan->n_sets = n_sets;
    plan->off_bytes = ((size_t)(n + 1) * sizeof(unsigned long long) + 15) / 16 * 16;
    plan->huff_bytes = (size_t)n_sets * 4 * sizeof(JpegHuff);
    plan->coef_bytes = (size_t)blocks * 128;
    plan->plane_bytes = (size_t)blocks * 64;
    plan->out_bytes = out_bytes;
    return IO_OK;
}

}  // namespace

extern "C" int io_jpeg_set_images_per_wave(int images) {
    IO_REQUIRE(images >= 1 && images <= 64, IO_ERR_SHAPE, "jpeg: images per wave %d (1..64)", images);
    g_images_per_wave.store(images);
    return IO_OK;
}
extern "C" int io_jpeg_get_images_per_wave(void) { return g_images_per_wave.load(); }
extern "C" int io_jpeg_lds_table_sets(void) { return IO_JPEG_LDS_TABLE_SETS; }

extern "C" size_t io_jpeg_workspace_bytes(const io_jpeg_desc* desc_host, int n) {
    JpegPlan plan;
    if (jpeg_check_desc(desc_host, n, &plan) != IO_OK) return 0;
    return plan.off_bytes + plan.huff_bytes + plan.coef_bytes + plan.plane_bytes;
}

namespace {

// what the parallel entropy stage adds behind the sequential workspace: subsequence offsets, fallback words, records
struct JpegParPlan {
    long total_sub;
    size_t suboff_bytes, fallback_bytes, rec_bytes;
};

int jpeg_check_par(const io_jpeg_desc* desc, int n, int subseq_bytes, JpegParPlan* par) {
    IO_REQUIRE(subseq_bytes >= JPEG_SYNC_MIN_BYTES && subseq_bytes <= JPEG_SYNC_MAX_BYTES && subseq_bytes % 8 == 0, IO_ERR_SHAPE,
               "jpeg_decode_par: subseq_bytes=%d (a multiple of 8 from %d to %d)", subseq_bytes, JPEG_SYNC_MIN_BYTES,
               JPEG_SYNC_MAX_BYTES);
    long total = 0;
    for (int i = 0; i < n; ++i) total += jpeg_sync_count(desc[i].data_bytes, subseq_bytes);
    par->total_sub = total;
    par->suboff_bytes = ((size_t)(n + 1) * sizeof(unsigned long long) + 15) / 16 * 16;
    par->fallback_bytes = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16;
    par->rec_bytes = (size_t)total * JS_WORDS * sizeof(uint32_t);
    return IO_OK;
}

// the checks of a decode call that need the buffers' sizes; the workspace size is left to the caller
int jpeg_check_call(const uint8_t* pool_dev, size_t pool_bytes, const io_jpeg_tables* tables_dev, const io_jpeg_tables* tables_host,
                    size_t tables_bytes, const io_jpeg_desc* desc_dev, const io_jpeg_desc* desc_host, int n, uint8_t* out,
                    size_t out_bytes, void* workspace, int32_t* status_dev, JpegPlan* planp) {
    IO_REQUIRE(pool_dev && tables_dev && tables_host && desc_dev && out && workspace && status_dev, IO_ERR_SHAPE,
               "jpeg_decode: null pointer");
    JpegPlan& plan = *planp;
    const int rc = jpeg_check_desc(desc_host, n, &plan);
    if (rc != IO_OK) return rc;
    IO_REQUIRE((size_t)plan.n_sets * sizeof(io_jpeg_tables) <= tables_bytes, IO_ERR_SHAPE,
               "jpeg_decode: table set %d outside the %zu table bytes", plan.n_sets - 1, tables_bytes);
    for (int s = 0; s < plan.n_sets; ++s) {
        JpegHuff h;
        for (int t = 0; t < 4; ++t)
            IO_REQUIRE(jpeg_build_huff(tables_host[s].huff_counts[t], tables_host[s].huff_symbols[t], &h), IO_ERR_SHAPE,
                       "jpeg_decode: table set %d, Huffman table %d: the code lengths form no prefix code of at most 256 symbols",
                       s, t);
    }
    for (int i = 0; i < n; ++i) {
        const io_jpeg_desc& d = desc_host[i];
        IO_REQUIRE((size_t)d.data_off <= pool_bytes && (size_t)d.data_bytes <= pool_bytes - (size_t)d.data_off, IO_ERR_SHAPE,
                   "jpeg_decode: image %d data outside the byte pool", i);
        const size_t nb = 3 * (size_t)d.H * (size_t)d.W;
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && nb <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "jpeg_decode: image %d output outside the output buffer", i);
    }
    IO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tables_dev & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0,
               IO_ERR_SHAPE, "jpeg_decode: workspace and tables must be 16-byte aligned, descriptors 8-byte aligned");
    return IO_OK;
}

// stages 2 and 3 behind either entropy stage
void jpeg_launch_pixels(const JpegPlan& plan, const io_jpeg_tables* tables_dev, const io_jpeg_desc* desc_dev,
                        const unsigned long long* off, const int16_t* coef, uint8_t* planes, uint8_t* out, int n, hipStream_t st) {
    {
        IoProfScope prof(IO_PROF_JPEG_IDCT, 0.0, (double)plan.coef_bytes + (double)plan.plane_bytes, st);
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(io_cdiv(plan.total_blocks, kThreads)), dim3(kThreads), 0, st, tables_dev,
                           desc_dev, off, coef, planes, n);
    }
    {
        IoProfScope prof(IO_PROF_JPEG_COLOUR, 0.0, (double)plan.plane_bytes + plan.out_bytes, st);
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3(io_cdiv(plan.max_words, kChunkWords), n), dim3(kThreads), 0, st, desc_dev,
                           off, planes, out);
    }
}

}  // namespace

extern "C" int io_jpeg_decode_u8(const uint8_t* pool_dev, size_t pool_bytes, const io_jpeg_tables* tables_dev,
                                 const io_jpeg_tables* tables_host, size_t tables_bytes, const io_jpeg_desc* desc_dev,
                                 const io_jpeg_desc* desc_host, int n, uint8_t* out, size_t out_bytes, void* workspace,
                                 size_t workspace_bytes, int32_t* status_dev, hipStream_t st) {
    JpegPlan plan;
    const int rc = jpeg_check_call(pool_dev, pool_bytes, tables_dev, tables_host, tables_bytes, desc_dev, desc_host, n, out,
                                   out_bytes, workspace, status_dev, &plan);
    if (rc != IO_OK) return rc;
    const size_t need = plan.off_bytes + plan.huff_bytes + plan.coef_bytes + plan.plane_bytes;
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "jpeg_decode: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws);
    JpegHuff* huff = reinterpret_cast<JpegHuff*>(ws + plan.off_bytes);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + plan.off_bytes + plan.huff_bytes);
    uint8_t* planes = ws + plan.off_bytes + plan.huff_bytes + plan.coef_bytes;
    const hipError_t e = hipMemsetAsync(coef, 0, plan.coef_bytes, st);
    IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "jpeg_decode: clearing the coefficients: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kThreads), 0, st, desc_dev, n, off);
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3(plan.n_sets), dim3(64), 0, st, tables_dev, huff);
    const int per_wave = g_images_per_wave.load();
    {
        IoProfScope prof(IO_PROF_JPEG_ENTROPY, 0.0, (double)pool_bytes + (double)plan.coef_bytes, st);
        const int waves = io_cdiv(n, per_wave);
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(io_cdiv(waves, kThreads / 64)), dim3(kThreads), 0, st, pool_dev, huff,
                           plan.n_sets, desc_dev, off, coef, status_dev, n, per_wave);
    }
    jpeg_launch_pixels(plan, tables_dev, desc_dev, off, coef, planes, out, n, st);
    return io_check_launch("jpeg_decode");
}

extern "C" size_t io_jpeg_par_workspace_bytes(const io_jpeg_desc* desc_host, int n, int subseq_bytes) {
    JpegPlan plan;
    JpegParPlan par;
    if (jpeg_check_desc(desc_host, n, &plan) != IO_OK || jpeg_check_par(desc_host, n, subseq_bytes, &par) != IO_OK) return 0;
    const size_t seq = plan.off_bytes + plan.huff_bytes + plan.coef_bytes + plan.plane_bytes;
    return (seq + 15) / 16 * 16 + par.suboff_bytes + par.fallback_bytes + par.rec_bytes;
}

extern "C" int io_jpeg_decode_par_u8(const uint8_t* pool_dev, size_t pool_bytes, const io_jpeg_tables* tables_dev,
                                     const io_jpeg_tables* tables_host, size_t tables_bytes, const io_jpeg_desc* desc_dev,
                                     const io_jpeg_desc* desc_host, int n, uint8_t* out, size_t out_bytes, void* workspace,
                                     size_t workspace_bytes, int32_t* status_dev, int subseq_bytes, int max_rounds,
                                     int32_t* info_dev, hipStream_t st) {
    JpegPlan plan;
    JpegParPlan par;
    int rc = jpeg_check_call(pool_dev, pool_bytes, tables_dev, tables_host, tables_bytes, desc_dev, desc_host, n, out, out_bytes,
                             workspace, status_dev, &plan);
    if (rc != IO_OK) return rc;
    rc = jpeg_check_par(desc_host, n, subseq_bytes, &par);
    if (rc != IO_OK) return rc;
    IO_REQUIRE(max_rounds >= 1 && max_rounds <= JPEG_SYNC_MAX_ROUNDS, IO_ERR_SHAPE, "jpeg_decode_par: max_rounds=%d (1..%d)",
               max_rounds, JPEG_SYNC_MAX_ROUNDS);
    const size_t seq = (plan.off_bytes + plan.huff_bytes + plan.coef_bytes + plan.plane_bytes + 15) / 16 * 16;
    const size_t need = seq + par.suboff_bytes + par.fallback_bytes + par.rec_bytes;
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "jpeg_decode_par: workspace of %zu bytes, %zu needed", workspace_bytes,
               need);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws);
    JpegHuff* huff = reinterpret_cast<JpegHuff*>(ws + plan.off_bytes);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + plan.off_bytes + plan.huff_bytes);
    uint8_t* planes = ws + plan.off_bytes + plan.huff_bytes + plan.coef_bytes;
    unsigned long long* suboff = reinterpret_cast<unsigned long long*>(ws + seq);
    int32_t* fallback = reinterpret_cast<int32_t*>(ws + seq + par.suboff_bytes);
    uint32_t* rec = reinterpret_cast<uint32_t*>(ws + seq + par.suboff_bytes + par.fallback_bytes);
    const hipError_t e = hipMemsetAsync(coef, 0, plan.coef_bytes, st);
    IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "jpeg_decode_par: clearing the coefficients: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kThreads), 0, st, desc_dev, n, off);
    hipLaunchKernelGGL(jpeg_sub_offsets_kernel, dim3(1), dim3(kThreads), 0, st, desc_dev, n, subseq_bytes, suboff);
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3(plan.n_sets), dim3(64), 0, st, tables_dev, huff);
    {
        // both launches in the class of the sequential stage: the fallback is part of what this stage costs
        IoProfScope prof(IO_PROF_JPEG_ENTROPY, 0.0, (double)pool_bytes + (double)plan.coef_bytes + (double)par.rec_bytes, st);
        hipLaunchKernelGGL(jpeg_sync_kernel, dim3(n), dim3(kThreads), 0, st, pool_dev, huff, desc_dev, off, suboff, rec, coef,
                           status_dev, fallback, info_dev, subseq_bytes, max_rounds);
        hipLaunchKernelGGL(jpeg_fallback_kernel, dim3(io_cdiv(n, kThreads / 64)), dim3(kThreads), 0, st, pool_dev, huff,
                           plan.n_sets, desc_dev, off, coef, status_dev, fallback, n);
    }
    jpeg_launch_pixels(plan, tables_dev, desc_dev, off, coef, planes, out, n, st);
    return io_check_launch("jpeg_decode_par");
}

// ---- progressive files (jpeg_prog.h) ---------------------------------------------------------------------------------------
namespace {

static_assert(sizeof(io_jpeg_prog_scan) == 64 && sizeof(io_jpeg_prog_image) == 16 && sizeof(io_jpeg_huff_raw) == 272,
              "ABI layout of the progressive JPEG tables");

__global__ __launch_bounds__(64) void jpeg_prog_tables_kernel(const io_jpeg_huff_raw* __restrict__ raw, JpegHuff* __restrict__ huff,
                                                              int n_huff) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n_huff) (void)jpeg_build_huff(raw[t].counts, raw[t].symbols, huff + t);
}

__device__ __forceinline__ int prog_run_scan(const io_jpeg_prog_scan& sc, const io_jpeg_desc& d, const uint8_t* __restrict__ pool,
                                             const JpegHuff* __restrict__ huff, int16_t* __restrict__ coef) {
    JpegProgScan s;
    s.data = pool + sc.data_off;
    s.nbytes = sc.data_bytes;
    s.n_scan_comp = sc.n_comp;
    s.comp = sc.comp[0];
    s.ss = sc.ss;
    s.se = sc.se;
    s.ah = sc.ah;
    s.al = sc.al;
    s.restart_interval = sc.restart_interval;
    const bool dc_refine = sc.ss == 0 && sc.ah != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) s.tab[j] = huff + (dc_refine || j >= sc.n_comp ? 0 : sc.table[j]);    // the host checked the indices
    s.W = d.W;
    s.H = d.H;
    s.n_comp = d.n_comp;
    s.hs = d.hs;
    s.vs = d.vs;
    return jpeg_prog_decode_scan(s, coef);
}

// One block per image.  concurrent: the block walks the image's levels, a barrier behind each; inside a level the ready scans
// are dealt to the four waves in turn and run on lane 0 of their wave (a level of more than four scans takes several turns of
// a wave).  Scans of one level touch disjoint coefficients (the host checked the levels), and a coefficient an earlier level
// stored is read behind that level's barrier.  The number of barriers is the image's n_levels for every thread and no thread
// returns in front of the last one.  Not concurrent: thread 0 runs the scans in file order, no barrier at all.
__global__ __launch_bounds__(kThreads) void jpeg_prog_entropy_kernel(const uint8_t* __restrict__ pool, const JpegHuff* __restrict__ huff,
                                                                     const io_jpeg_desc* __restrict__ desc,
                                                                     const io_jpeg_prog_image* __restrict__ images,
                                                                     const io_jpeg_prog_scan* __restrict__ scans,
                                                                     const unsigned long long* __restrict__ off,
                                                                     int16_t* __restrict__ coef, int32_t* __restrict__ scan_status,
                                                                     int32_t* __restrict__ status, int concurrent) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const io_jpeg_prog_image im = images[img];
    const io_jpeg_desc d = desc[img];
    int16_t* dst = coef + 64 * (long)off[img];
    const io_jpeg_prog_scan* mine = scans + im.first_scan;
    int32_t* mine_status = scan_status + im.first_scan;
    if (!concurrent) {                                           // block-uniform
        if (tid == 0) {
            int first = 0;
            for (int s = 0; s < im.n_scans; ++s) {
                const int st = prog_run_scan(mine[s], d, pool, huff, dst);
                if (first == 0) first = st;
            }
            status[img] = first;
        }
        return;
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (int level = 0; level < im.n_levels; ++level) {          // block-uniform trip count
        if (lane == 0) {
            int seen = 0;
            for (int s = 0; s < im.n_scans; ++s) {
                if (mine[s].level != level) continue;
                if ((seen++ & (kThreads / 64 - 1)) == wave) mine_status[s] = prog_run_scan(mine[s], d, pool, huff, dst);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int first = 0;
        for (int s = 0; s < im.n_scans && first == 0; ++s) first = mine_status[s];
        status[img] = first;
    }
}

struct JpegProgPlan {
    size_t huff_bytes, scan_status_bytes;
};

int jpeg_prog_plan(int n_huff, int n_scans, JpegProgPlan* pp) {
    IO_REQUIRE(n_huff >= 1 && n_huff <= 65535, IO_ERR_SHAPE, "jpeg_decode_prog: n_huff=%d (1..65535 Huffman tables)", n_huff);
    IO_REQUIRE(n_scans >= 1 && n_scans <= (1 << 24), IO_ERR_SHAPE, "jpeg_decode_prog: n_scans=%d (1..2^24)", n_scans);
    pp->huff_bytes = ((size_t)n_huff * sizeof(JpegHuff) + 15) / 16 * 16;
    pp->scan_status_bytes = ((size_t)n_scans * sizeof(int32_t) + 15) / 16 * 16;
    return IO_OK;
}

// the scan rules of DESIGN.md "Progressive JPEG" and the level rule, on the host tables
int jpeg_prog_check_scans(const io_jpeg_desc* desc, const io_jpeg_prog_image* images, int n, const io_jpeg_prog_scan* scans, int n_scans,
                          const io_jpeg_huff_raw* huff_host, int n_huff, size_t pool_bytes) {
    std::vector<uint8_t> used((size_t)n_huff, 0);
    long next = 0;
    for (int i = 0; i < n; ++i) {
        const io_jpeg_prog_image& im = images[i];
        const io_jpeg_desc& d = desc[i];
        IO_REQUIRE(im.first_scan == next && im.n_scans >= 1 && im.n_scans <= n_scans - next, IO_ERR_SHAPE,
                   "jpeg_decode_prog: image %d has scans [%d, %d + %d): the ranges must follow each other inside the %d scans", i,
                   im.first_scan, im.first_scan, im.n_scans, n_scans);
        IO_REQUIRE(im.n_levels >= 1 && im.n_levels <= im.n_scans, IO_ERR_SHAPE, "jpeg_decode_prog: image %d has n_levels=%d for %d scans",
                   i, im.n_levels, im.n_scans);
        next += im.n_scans;
        int al_of[3][64], level_of[3][64];                       // per coefficient: the Al it was sent down to, the level of its last scan
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 64; ++k) al_of[c][k] = level_of[c][k] = -1;
        for (int s = 0; s < im.n_scans; ++s) {
            const int g = im.first_scan + s;
            const io_jpeg_prog_scan& sc = scans[g];
            IO_REQUIRE(sc.image == i, IO_ERR_SHAPE, "jpeg_decode_prog: scan %d names image %d inside the range of image %d", g, sc.image, i);
            IO_REQUIRE(sc.n_comp >= 1 && sc.n_comp <= 3 && (sc.n_comp == 1 || sc.n_comp == d.n_comp), IO_ERR_SHAPE,
                       "jpeg_decode_prog: scan %d has %d of the image's %d components (1 or all)", g, sc.n_comp, d.n_comp);
            for (int j = 0; j < sc.n_comp; ++j)
                IO_REQUIRE(sc.comp[j] < d.n_comp && (j == 0 || sc.comp[j] > sc.comp[j - 1]), IO_ERR_SHAPE,
                           "jpeg_decode_prog: scan %d component list is not in increasing frame order below %d", g, d.n_comp);
            IO_REQUIRE(sc.ss <= sc.se && sc.se <= 63 && (sc.ss == 0 ? sc.se == 0 : sc.n_comp == 1), IO_ERR_SHAPE,
                       "jpeg_decode_prog: scan %d has Ss=%d Se=%d with %d components (a DC scan Ss = Se = 0, an AC scan one component and "
                       "1 <= Ss <= Se <= 63)", g, sc.ss, sc.se, sc.n_comp);
            IO_REQUIRE(sc.al <= 13 && (sc.ah == 0 || sc.ah == sc.al + 1), IO_ERR_SHAPE,
                       "jpeg_decode_prog: scan %d has Ah=%d Al=%d (Al <= 13; Ah 0 or Al + 1)", g, sc.ah, sc.al);
            IO_REQUIRE(sc.restart_interval >= 0, IO_ERR_SHAPE, "jpeg_decode_prog: scan %d has restart_interval=%d", g, sc.restart_interval);
            IO_REQUIRE(sc.level >= 0 && sc.level < im.n_levels, IO_ERR_SHAPE, "jpeg_decode_prog: scan %d has level %d of %d", g, sc.level,
                       im.n_levels);
            IO_REQUIRE(sc.data_off >= 0 && sc.data_bytes >= 0 && (size_t)sc.data_off <= pool_bytes &&
                           (size_t)sc.data_bytes <= pool_bytes - (size_t)sc.data_off,
                       IO_ERR_SHAPE, "jpeg_decode_prog: scan %d data outside the byte pool", g);
            for (int j = 0; j < sc.n_comp; ++j) {
                const int c = sc.comp[j];
                IO_REQUIRE(sc.ss == 0 || al_of[c][0] >= 0, IO_ERR_SHAPE,
                           "jpeg_decode_prog: scan %d is an AC scan of component %d in front of its first DC scan", g, c);
                for (int k = sc.ss; k <= sc.se; ++k) {
                    IO_REQUIRE(sc.ah == 0 ? al_of[c][k] < 0 : al_of[c][k] == sc.ah, IO_ERR_SHAPE,
                               "jpeg_decode_prog: scan %d (Ah=%d) meets coefficient %d of component %d at Al=%d (a first scan: not sent "
                               "before; a refinement: Ah = the previous Al)", g, sc.ah, k, c, al_of[c][k]);
                    IO_REQUIRE(sc.level > level_of[c][k], IO_ERR_SHAPE,
                               "jpeg_decode_prog: scan %d has level %d, not above level %d of an earlier scan that shares coefficient %d "
                               "of component %d", g, sc.level, level_of[c][k], k, c);
                    al_of[c][k] = sc.al;
                    level_of[c][k] = sc.level;
                }
                if (!(sc.ss == 0 && sc.ah != 0)) {
                    IO_REQUIRE(sc.table[j] >= 0 && sc.table[j] < n_huff, IO_ERR_SHAPE,
                               "jpeg_decode_prog: scan %d names Huffman table %d outside the pool of %d", g, sc.table[j], n_huff);
                    used[(size_t)sc.table[j]] = 1;
                }
            }
        }
        for (int c = 0; c < d.n_comp; ++c)
            for (int k = 0; k < 64; ++k)
                IO_REQUIRE(al_of[c][k] == 0, IO_ERR_SHAPE,
                           "jpeg_decode_prog: image %d is an incomplete progression: coefficient %d of component %d %s", i, k, c,
                           al_of[c][k] < 0 ? "is never sent" : "is not refined down to Al = 0");
    }
    IO_REQUIRE(next == n_scans, IO_ERR_SHAPE, "jpeg_decode_prog: the images name %ld of the %d scans", next, n_scans);
    for (int t = 0; t < n_huff; ++t) {
        if (!used[(size_t)t]) continue;
        JpegHuff h;
        IO_REQUIRE(jpeg_build_huff(huff_host[t].counts, huff_host[t].symbols, &h), IO_ERR_SHAPE,
                   "jpeg_decode_prog: Huffman table %d: the code lengths form no prefix code of at most 256 symbols", t);
    }
    return IO_OK;
}

}  // namespace

extern "C" size_t io_jpeg_prog_workspace_bytes(const io_jpeg_desc* desc_host, int n, int n_huff, int n_scans) {
    JpegPlan plan;
    JpegProgPlan pp;
    if (jpeg_check_desc(desc_host, n, &plan) != IO_OK || jpeg_prog_plan(n_huff, n_scans, &pp) != IO_OK) return 0;
    return plan.off_bytes + pp.huff_bytes + plan.coef_bytes + plan.plane_bytes + pp.scan_status_bytes;
}

extern "C" int io_jpeg_decode_prog_u8(const uint8_t* pool_dev, size_t pool_bytes, const io_jpeg_tables* tables_dev,
                                      const io_jpeg_tables* tables_host, size_t tables_bytes, const io_jpeg_huff_raw* huff_dev,
                                      const io_jpeg_huff_raw* huff_host, int n_huff, const io_jpeg_desc* desc_dev,
                                      const io_jpeg_desc* desc_host, const io_jpeg_prog_image* image_dev,
                                      const io_jpeg_prog_image* image_host, int n, const io_jpeg_prog_scan* scan_dev,
                                      const io_jpeg_prog_scan* scan_host, int n_scans, uint8_t* out, size_t out_bytes, void* workspace,
                                      size_t workspace_bytes, int32_t* status_dev, int concurrent, hipStream_t st) {
    IO_REQUIRE(pool_dev && tables_dev && tables_host && huff_dev && huff_host && desc_dev && desc_host && image_dev && image_host &&
                   scan_dev && scan_host && out && workspace && status_dev,
               IO_ERR_SHAPE, "jpeg_decode_prog: null pointer");
    IO_REQUIRE(concurrent == 0 || concurrent == 1, IO_ERR_SHAPE, "jpeg_decode_prog: concurrent=%d (0 or 1)", concurrent);
    JpegPlan plan;
    JpegProgPlan pp;
    int rc = jpeg_check_desc(desc_host, n, &plan);
    if (rc != IO_OK) return rc;
    rc = jpeg_prog_plan(n_huff, n_scans, &pp);
    if (rc != IO_OK) return rc;
    IO_REQUIRE((size_t)plan.n_sets * sizeof(io_jpeg_tables) <= tables_bytes, IO_ERR_SHAPE,
               "jpeg_decode_prog: table set %d outside the %zu table bytes", plan.n_sets - 1, tables_bytes);
    for (int i = 0; i < n; ++i) {
        const io_jpeg_desc& d = desc_host[i];
        const size_t nb = 3 * (size_t)d.H * (size_t)d.W;
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && nb <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "jpeg_decode_prog: image %d output outside the output buffer", i);
    }
    rc = jpeg_prog_check_scans(desc_host, image_host, n, scan_host, n_scans, huff_host, n_huff, pool_bytes);
    if (rc != IO_OK) return rc;
    IO_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)tables_dev & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0 &&
                   ((uintptr_t)scan_dev & 7) == 0 && ((uintptr_t)image_dev & 3) == 0,
               IO_ERR_SHAPE,
               "jpeg_decode_prog: workspace and tables must be 16-byte aligned, descriptors and scans 8-byte, image records 4-byte aligned");
    const size_t need = plan.off_bytes + pp.huff_bytes + plan.coef_bytes + plan.plane_bytes + pp.scan_status_bytes;
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "jpeg_decode_prog: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    unsigned long long* off = reinterpret_cast<unsigned long long*>(ws);
    JpegHuff* huff = reinterpret_cast<JpegHuff*>(ws + plan.off_bytes);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + plan.off_bytes + pp.huff_bytes);
    uint8_t* planes = ws + plan.off_bytes + pp.huff_bytes + plan.coef_bytes;
    int32_t* scan_status = reinterpret_cast<int32_t*>(planes + plan.plane_bytes);
    const hipError_t e = hipMemsetAsync(coef, 0, plan.coef_bytes, st);
    IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "jpeg_decode_prog: clearing the coefficients: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kThreads), 0, st, desc_dev, n, off);
    hipLaunchKernelGGL(jpeg_prog_tables_kernel, dim3(io_cdiv(n_huff, 64)), dim3(64), 0, st, huff_dev, huff, n_huff);
    {
        IoProfScope prof(IO_PROF_JPEG_PROG_ENTROPY, 0.0, (double)pool_bytes + (double)plan.coef_bytes, st);
        hipLaunchKernelGGL(jpeg_prog_entropy_kernel, dim3(n), dim3(kThreads), 0, st, pool_dev, huff, desc_dev, image_dev, scan_dev, off, coef,
                           scan_status, status_dev, concurrent);
    }
    jpeg_launch_pixels(plan, tables_dev, desc_dev, off, coef, planes, out, n, st);
    return io_check_launch("jpeg_decode_prog");
}
