// Mask relations and per-instance disparity statistics of one image on the device: what the reference's order rules of
// tools/test.py recompute pair by pair on the host (inference.py: bordering, infer_gt_order, the area / y-axis baselines,
// net_forward_midas_pretrained).
//
// io_mask_pack         uint8 masks [n][H][W] -> bit images [n][H][ceil(W/32)] of `m != 0` or `m == 1`, optionally dilated
//                      once with the 3x3 cross (cv2.dilate of inference.bordering), and optionally the exact int64
//                      statistics of each mask.  One block per (row, mask); each wave turns 64 pixels into two words by
//                      one ballot.
// io_mask_pair_counts  counts[i][j] = popcount(P_i AND Q_j) over the image for two sets of bit images.  Blocks are tiles of
//                      16 P masks x 16 Q masks x a range of words; both tiles are staged in LDS, one (i, j) per thread,
//                      the integer partials are added into counts (zeroed first), so any order gives the same result.
// io_instance_depth_select
//                      per instance i: V_i = 1 / (disp + 1e-6) where mask_i != 0; k = |V_i|; lo / hi = torch.quantile(V_i,
//                      0.05 / 0.95) (linear rule); median = clamp(lower median, lo, hi) or mean = mean(clamp(V_i, lo, hi)).
//                      Exact order statistics by a three-digit radix select (the machinery of depth_eval.hip), for all n
//                      instances at once: grid = blocks-per-map x n, four launches for the median, six for the mean.
#include "io_common.h"

#include <math.h>

// Elementwise steps round like the reference's fp32 torch expressions: plain operators under contract(off); the one fused
// multiply-add of torch.lerp is written out as fmaf.
#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// io_mask_pack
constexpr int kPT = 256;

__device__ __forceinline__ bool mpred(unsigned v, int eq1) { return eq1 ? v == 1u : v != 0u; }

__global__ __launch_bounds__(kPT) void mask_pack_kernel(const uint8_t* __restrict__ m, int H, int W, int Wq, int eq1,
                                                        int dilate, uint32_t* __restrict__ bits,
                                                        long long* __restrict__ stats) {
    __shared__ long long sred[kPT / 64][4];
    const int y = blockIdx.x, i = blockIdx.y;
    const size_t plane = (size_t)H * W;
    const uint8_t* mi = m + (size_t)i * plane;
    const uint8_t* row = mi + (size_t)y * W;
    uint32_t* brow = bits + ((size_t)i * H + y) * Wq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long s_sum = 0, s_one = 0, s_nz = 0;
    // every wave of the block runs the same number of iterations, so the ballot sees whole waves
    for (int x0 = 0; x0 < W; x0 += kPT) {
        const int x = x0 + threadIdx.x;
        bool p = false;
        if (x < W) {
            const unsigned v = row[x];
            s_sum += v;
            s_one += v == 1u;
            s_nz += v != 0u;
            p = mpred(v, eq1);
            if (dilate) {
                if (y > 0) p |= mpred(row[x - W], eq1);
                if (y + 1 < H) p |= mpred(row[x + W], eq1);
                if (x > 0) p |= mpred(row[x - 1], eq1);
                if (x + 1 < W) p |= mpred(row[x + 1], eq1);
            }
        }
        const unsigned long long b = __ballot(p);
        const int word = (x0 + wave * 64) >> 5;          // first of the wave's two words
        if (lane == 0 && word < Wq) brow[word] = (uint32_t)b;
        if (lane == 32 && word + 1 < Wq) brow[word + 1] = (uint32_t)(b >> 32);
    }
    if (!stats) return;
    for (int o = 32; o > 0; o >>= 1) {
        s_sum += __shfl_xor(s_sum, o);
        s_one += __shfl_xor(s_one, o);
        s_nz += __shfl_xor(s_nz, o);
    }
    if (lane == 0) {
        sred[wave][0] = s_sum;
        sred[wave][1] = s_one;
        sred[wave][2] = s_nz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = 0, b = 0, c = 0;
        for (int k = 0; k < kPT / 64; ++k) {
            a += sred[k][0];
            b += sred[k][1];
            c += sred[k][2];
        }
        unsigned long long* st = reinterpret_cast<unsigned long long*>(stats) + (size_t)i * 4;
        if (a) atomicAdd(st + 0, (unsigned long long)a);
        if (b) {
            atomicAdd(st + 1, (unsigned long long)b);
            atomicAdd(st + 2, (unsigned long long)(b * y));
        }
        if (c) atomicAdd(st + 3, (unsigned long long)c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// io_mask_pair_counts
constexpr int kCT = 256;
constexpr int kTI = 16, kTJ = 16;   // masks per tile side: one (i, j) per thread
constexpr int kCW = 128;            // words per LDS chunk
constexpr int kCWp = kCW + 1;       // padded row: the 16 j of a wave read 16 different banks
static_assert(kTI == kTJ && kTI * kTJ == kCT, "one (i, j) per thread; both tiles staged by one loop");

__global__ __launch_bounds__(kCT) void pair_counts_kernel(const uint32_t* __restrict__ P, int np, const uint32_t* __restrict__ Q,
                                                          int nq, long L, long per_block, int* __restrict__ counts) {
    __shared__ uint32_t sp[kTI][kCWp], sq[kTJ][kCWp];
    const int i0 = blockIdx.y * kTI, j0 = blockIdx.z * kTJ;
    const long w_beg = (long)blockIdx.x * per_block;
    const long w_end = w_beg + per_block < L ? w_beg + per_block : L;
    const int ti = threadIdx.x / kTJ, tj = threadIdx.x % kTJ;
    unsigned acc = 0;
    for (long c0 = w_beg; c0 < w_end; c0 += kCW) {
        const int cw = (int)(w_end - c0 < kCW ? w_end - c0 : kCW);
        for (int e = threadIdx.x; e < kTI * kCW; e += kCT) {
            const int r = e / kCW, w = e % kCW;
            const int gi = i0 + r, gj = j0 + r;
            sp[r][w] = (w < cw && gi < np) ? P[(size_t)gi * L + c0 + w] : 0u;
            sq[r][w] = (w < cw && gj < nq) ? Q[(size_t)gj * L + c0 + w] : 0u;
        }
        __syncthreads();
#pragma unroll 8
        for (int w = 0; w < kCW; ++w) acc += __popc(sp[ti][w] & sq[tj][w]);
        __syncthreads();
    }
    const int gi = i0 + ti, gj = j0 + tj;
    if (acc && gi < np && gj < nq) atomicAdd(counts + (size_t)gi * nq + gj, (int)acc);
}

// ---------------------------------------------------------------------------------------------------------------------
// io_instance_depth_select
constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kMaxBlk = 64;         // blocks per map
constexpr int kBins = 2048;
constexpr int kTg = 5;              // targets: floor / ceil of the 5 % rank, floor / ceil of the 95 % rank, the lower median
// per instance: pass-1 histogram, kTg pass-2 histograms (11 bits), kTg pass-3 histograms (10 bits)
constexpr int kHistWords = kBins + kTg * kBins + kTg * 1024;

int ds_blocks(long N) {
    long b = (N + kT * 8 - 1) / (kT * 8);
    return (int)(b < 1 ? 1 : (b > kMaxBlk ? kMaxBlk : b));
}

struct DsWs {
    unsigned* hist;    // [n][kHistWords]
    unsigned* state;   // [n][2][kTg][2]: (prefix, rank in bucket) after pass 1 / pass 2
    float* stat;       // [n][4]: lo, hi, clamped lower median, (unused)
    int* cnt;          // [n]
    double* sums;      // [n][nb]
};

size_t al(size_t x) { return (x + 255) / 256 * 256; }

// the histograms come first: they are the only part that is zeroed before the passes
size_t ds_hist_bytes(int n) { return al((size_t)n * kHistWords * 4); }

size_t ds_layout(int n, int nb, char* base, DsWs* w) {
    const size_t s_hist = ds_hist_bytes(n), s_state = al((size_t)n * 2 * kTg * 2 * 4), s_stat = al((size_t)n * 4 * 4),
                 s_cnt = al((size_t)n * 4), s_sums = al((size_t)n * nb * 8);
    if (w) {
        w->hist = reinterpret_cast<unsigned*>(base);
        w->state = reinterpret_cast<unsigned*>(base + s_hist);
        w->stat = reinterpret_cast<float*>(base + s_hist + s_state);
        w->cnt = reinterpret_cast<int*>(base + s_hist + s_state + s_stat);
        w->sums = reinterpret_cast<double*>(base + s_hist + s_state + s_stat + s_cnt);
    }
    return s_hist + s_state + s_stat + s_cnt + s_sums;
}

__device__ __forceinline__ unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// depth = 1 / (pred_disp + 1e-6) in fp32 (inference.net_forward_midas_pretrained)
__device__ __forceinline__ float to_depth(float d) { return __fdiv_rn(1.f, d + 1e-6f); }

// torch.quantile's linear rule for k values: rank = fp32(q) * (k - 1) in fp32, below = floor, above = ceil
__device__ __forceinline__ float q_rank(float q, int k) { return q * (float)(k - 1); }
__device__ __forceinline__ unsigned q_below(float r, int k) {
    const unsigned b = (unsigned)r;
    return b > (unsigned)(k - 1) ? (unsigned)(k - 1) : b;
}
__device__ __forceinline__ unsigned q_above(float r, int k) {
    const unsigned a = (unsigned)ceilf(r);
    return a > (unsigned)(k - 1) ? (unsigned)(k - 1) : a;
}
__device__ __forceinline__ unsigned target_rank(int t, int k) {
    if (t == 4) return (unsigned)((k - 1) / 2);
    const float r = q_rank(t < 2 ? 0.05f : 0.95f, k);
    return (t & 1) ? q_above(r, k) : q_below(r, k);
}
// torch.lerp (ATen/native/Lerp.h): weight < 0.5 ? a + w * (b - a) : b - (b - a) * (1 - w), each as one fused multiply-add
__device__ __forceinline__ float t_lerp(float a, float b, float wt) {
    const float d = b - a;
    return fabsf(wt) < 0.5f ? fmaf(wt, d, a) : fmaf(-d, 1.f - wt, b);
}
__device__ __forceinline__ float t_clamp(float v, float lo, float hi) {
    // torch.clamp with tensor bounds: min(max(v, lo), hi), NaN propagating
    if (isnan(v) || isnan(lo) || isnan(hi)) return NAN;
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

__device__ __forceinline__ double wsumd(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Rank k (0-based) among the elements counted by h[nbins] (global): out[0] = its bucket, out[1] = its rank inside the
// bucket.  Block-cooperative (all kT threads), as in depth_eval.hip.  Also returns the total count in out[2].
__device__ void radix_find(const unsigned* __restrict__ h, int nbins, unsigned k, unsigned* out, unsigned* wtot) {
    const int per = nbins / kT;
    unsigned loc[8];
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        loc[j] = j < per ? h[threadIdx.x * per + j] : 0u;
        s += loc[j];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = s;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned excl = inc - s;
    for (int w = 0; w < wave; ++w) excl += wtot[w];
    if (k >= excl && k - excl < s) {          // exactly one thread holds rank k
        unsigned c = excl;
        bool done = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!done && j < per && k < c + loc[j]) {
                out[0] = threadIdx.x * per + j;
                out[1] = k - c;
                done = true;
            }
            c += loc[j];
        }
    }
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < kWaves; ++w) t += wtot[w];
        out[2] = t;
    }
    __syncthreads();
}

// ---- launch 1: 11-bit histogram of the top digit of V_i (its total is k) ----
__global__ __launch_bounds__(kT) void ds_pass1_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ masks, int N,
                                                      DsWs w) {
    __shared__ unsigned sh[kBins];
    const int i = blockIdx.y, nb = gridDim.x;
    for (int e = threadIdx.x; e < kBins; e += kT) sh[e] = 0u;
    __syncthreads();
    const uint8_t* m = masks + (size_t)i * N;
    for (int e = blockIdx.x * kT + threadIdx.x; e < N; e += nb * kT)
        if (m[e]) atomicAdd(&sh[fkey(to_depth(disp[e])) >> 21], 1u);
    __syncthreads();
    unsigned* hs = w.hist + (size_t)i * kHistWords;
    for (int e = threadIdx.x; e < kBins; e += kT) {
        const unsigned v = sh[e];
        if (v) atomicAdd(hs + e, v);
    }
}

// ---- launches 2 and 3: q = 1 -> 11-bit histograms of bits 20..10 inside each target's bucket; q = 2 -> bits 9..0 ----
__global__ __launch_bounds__(kT) void ds_pass_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ masks, int N,
                                                     int q, DsWs w) {
    __shared__ unsigned sh[kTg][kBins];
    __shared__ unsigned sel[3], wtot[kWaves], spre[kTg];
    __shared__ int sk;
    const int i = blockIdx.y, nb = gridDim.x;
    unsigned* hs = w.hist + (size_t)i * kHistWords;
    unsigned* st = w.state + (size_t)i * 2 * kTg * 2;
    if (q == 1) {
        radix_find(hs, kBins, 0u, sel, wtot);        // only for the total
        if (threadIdx.x == 0) {
            sk = (int)sel[2];
            if (blockIdx.x == 0) w.cnt[i] = sk;
        }
        __syncthreads();
    } else {
        if (threadIdx.x == 0) sk = w.cnt[i];
        __syncthreads();
    }
    const int k = sk;
    if (k <= 0) return;
    for (int t = 0; t < kTg; ++t) {
        const unsigned* h = q == 1 ? hs : hs + kBins + t * kBins;
        const unsigned r = q == 1 ? target_rank(t, k) : st[t * 2 + 1];
        radix_find(h, kBins, r, sel, wtot);
        if (threadIdx.x == 0) {
            spre[t] = q == 1 ? sel[0] : (st[t * 2] << 11) | sel[0];
            if (blockIdx.x == 0) {            // slot q - 1 is read by the next launch only
                st[kTg * 2 * (q - 1) + t * 2] = spre[t];
                st[kTg * 2 * (q - 1) + t * 2 + 1] = sel[1];
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < kTg * kBins; e += kT) (&sh[0][0])[e] = 0u;
    __syncthreads();
    unsigned pre[kTg];
#pragma unroll
    for (int t = 0; t < kTg; ++t) pre[t] = spre[t];
    const int pshift = q == 1 ? 21 : 10, dshift = q == 1 ? 10 : 0;
    const unsigned dmask = q == 1 ? 0x7ffu : 0x3ffu;
    const uint8_t* m = masks + (size_t)i * N;
    for (int e = blockIdx.x * kT + threadIdx.x; e < N; e += nb * kT) {
        if (!m[e]) continue;
        const unsigned key = fkey(to_depth(disp[e]));
#pragma unroll
        for (int t = 0; t < kTg; ++t)
            if ((key >> pshift) == pre[t]) atomicAdd(&sh[t][(key >> dshift) & dmask], 1u);
    }
    __syncthreads();
    unsigned* dst = hs + (q == 1 ? kBins : kBins + kTg * kBins);
    const int nbin = q == 1 ? kBins : 1024;
    for (int t = 0; t < kTg; ++t)
        for (int e = threadIdx.x; e < nbin; e += kT) {
            const unsigned v = sh[t][e];
            if (v) atomicAdd(dst + t * nbin + e, v);
        }
}

// ---- launch 4 (one block per instance): exact order statistics -> lo, hi, k and the median value ----
__global__ __launch_bounds__(kT) void ds_resolve_kernel(DsWs w, int median, float* __restrict__ value, float* __restrict__ lo,
                                                        float* __restrict__ hi, int* __restrict__ kout) {
    __shared__ unsigned sel[3], wtot[kWaves];
    __shared__ float sval[kTg];
    const int i = blockIdx.x;
    const int k = w.cnt[i];
    if (k <= 0) {
        if (threadIdx.x == 0) {
            w.stat[i * 4] = w.stat[i * 4 + 1] = w.stat[i * 4 + 2] = NAN;
            value[i] = NAN;
            if (lo) lo[i] = NAN;
            if (hi) hi[i] = NAN;
            if (kout) kout[i] = 0;
        }
        return;
    }
    const unsigned* h3 = w.hist + (size_t)i * kHistWords + kBins + kTg * kBins;
    const unsigned* st = w.state + (size_t)i * 2 * kTg * 2 + kTg * 2;
    for (int t = 0; t < kTg; ++t) {
        radix_find(h3 + t * 1024, 1024, st[t * 2 + 1], sel, wtot);
        if (threadIdx.x == 0) sval[t] = fkey_inv((st[t * 2] << 10) | sel[0]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float r5 = q_rank(0.05f, k), r95 = q_rank(0.95f, k);
    const float l = t_lerp(sval[0], sval[1], r5 - (float)q_below(r5, k));
    const float h = t_lerp(sval[2], sval[3], r95 - (float)q_below(r95, k));
    const float med = t_clamp(sval[4], l, h);
    w.stat[i * 4] = l;
    w.stat[i * 4 + 1] = h;
    w.stat[i * 4 + 2] = med;
    if (median) value[i] = med;
    if (lo) lo[i] = l;
    if (hi) hi[i] = h;
    if (kout) kout[i] = k;
}

// ---- launch 5 (mean): per-block fp64 sums of clamp(V_i, lo, hi) ----
__global__ __launch_bounds__(kT) void ds_sum_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ masks, int N,
                                                    DsWs w) {
    __shared__ double sred[kWaves];
    const int i = blockIdx.y, nb = gridDim.x;
    if (w.cnt[i] <= 0) return;
    const float l = w.stat[i * 4], h = w.stat[i * 4 + 1];
    const uint8_t* m = masks + (size_t)i * N;
    double acc = 0.0;
    for (int e = blockIdx.x * kT + threadIdx.x; e < N; e += nb * kT)
        if (m[e]) acc += (double)t_clamp(to_depth(disp[e]), l, h);
    acc = wsumd(acc);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sred[0];
        for (int k = 1; k < kWaves; ++k) s += sred[k];
        w.sums[(size_t)i * nb + blockIdx.x] = s;
    }
}

// ---- launch 6 (mean): fold the per-block sums in block order ----
__global__ __launch_bounds__(64) void ds_mean_kernel(DsWs w, int n, int nb, float* __restrict__ value) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int k = w.cnt[i];
    if (k <= 0) {
        value[i] = NAN;
        return;
    }
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += w.sums[(size_t)i * nb + b];
    value[i] = (float)(s / (double)k);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int io_mask_pack(const uint8_t* masks, int n, int H, int W, int predicate, int dilate, uint32_t* bits,
                            int64_t* stats, hipStream_t st) {
    IO_REQUIRE(n > 0 && n <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31) && H <= (1 << 30), IO_ERR_SHAPE,
               "mask_pack: n=%d H=%d W=%d", n, H, W);
    IO_REQUIRE(predicate == IO_MASK_NONZERO || predicate == IO_MASK_EQ1, IO_ERR_SHAPE, "mask_pack: predicate=%d", predicate);
    IO_REQUIRE(masks && bits, IO_ERR_SHAPE, "mask_pack: null pointer");
    const int Wq = io_cdiv(W, 32);
    if (stats) {
        const hipError_t e = hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(int64_t), st);
        IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "mask_pack: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(mask_pack_kernel, dim3(H, n), dim3(kPT), 0, st, masks, H, W, Wq, predicate == IO_MASK_EQ1 ? 1 : 0,
                       dilate ? 1 : 0, bits, reinterpret_cast<long long*>(stats));
    return io_check_launch("mask_pack");
}

extern "C" int io_mask_pair_counts(const uint32_t* p_bits, int n_p, const uint32_t* q_bits, int n_q, int H, int W,
                                   int32_t* counts, hipStream_t st) {
    IO_REQUIRE(n_p > 0 && n_q > 0 && n_p <= IO_MASK_MAX_N && n_q <= IO_MASK_MAX_N && H > 0 && W > 0 &&
                   (long)H * W < (1L << 31),
               IO_ERR_SHAPE, "mask_pair_counts: n_p=%d n_q=%d H=%d W=%d", n_p, n_q, H, W);
    IO_REQUIRE(p_bits && q_bits && counts, IO_ERR_SHAPE, "mask_pair_counts: null pointer");
    const long L = (long)H * io_cdiv(W, 32);
    const int bi = io_cdiv(n_p, kTI), bj = io_cdiv(n_q, kTJ);
    // enough word ranges for about 2048 blocks, each at least one LDS chunk long
    long splits = (2048 + (long)bi * bj - 1) / ((long)bi * bj);
    const long chunks = (L + kCW - 1) / kCW;
    if (splits > chunks) splits = chunks;
    if (splits < 1) splits = 1;
    const long per_block = (chunks + splits - 1) / splits * kCW;
    const int nsplit = (int)((L + per_block - 1) / per_block);
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_p * n_q * sizeof(int32_t), st);
    IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "mask_pair_counts: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(pair_counts_kernel, dim3(nsplit, bi, bj), dim3(kCT), 0, st, p_bits, n_p, q_bits, n_q, L, per_block,
                       counts);
    return io_check_launch("mask_pair_counts");
}

extern "C" size_t io_instance_depth_select_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    return ds_layout(n, ds_blocks((long)H * W), nullptr, nullptr);
}

extern "C" int io_instance_depth_select(const float* disp, int H, int W, const uint8_t* masks, int n, int method, float* value,
                                        float* lo, float* hi, int32_t* k, void* workspace, size_t workspace_bytes,
                                        hipStream_t st) {
    IO_REQUIRE(n > 0 && n <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31), IO_ERR_SHAPE,
               "instance_depth_select: n=%d H=%d W=%d", n, H, W);
    IO_REQUIRE(method == IO_DEPTH_SELECT_MEAN || method == IO_DEPTH_SELECT_MEDIAN, IO_ERR_SHAPE,
               "instance_depth_select: method=%d", method);
    IO_REQUIRE(disp && masks && value, IO_ERR_SHAPE, "instance_depth_select: null pointer");
    IO_REQUIRE(workspace && workspace_bytes >= io_instance_depth_select_workspace_bytes(n, H, W), IO_ERR_WORKSPACE,
               "instance_depth_select: workspace too small");
    const int N = H * W, nb = ds_blocks(N);
    DsWs w;
    ds_layout(n, nb, static_cast<char*>(workspace), &w);
    const hipError_t e = hipMemsetAsync(w.hist, 0, ds_hist_bytes(n), st);
    IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "instance_depth_select: %s", hipGetErrorString(e));
    const dim3 grid(nb, n);
    const int median = method == IO_DEPTH_SELECT_MEDIAN;
    hipLaunchKernelGGL(ds_pass1_kernel, grid, dim3(kT), 0, st, disp, masks, N, w);
    hipLaunchKernelGGL(ds_pass_kernel, grid, dim3(kT), 0, st, disp, masks, N, 1, w);
    hipLaunchKernelGGL(ds_pass_kernel, grid, dim3(kT), 0, st, disp, masks, N, 2, w);
    hipLaunchKernelGGL(ds_resolve_kernel, dim3(n), dim3(kT), 0, st, w, median, value, lo, hi, k);
    if (!median) {
        hipLaunchKernelGGL(ds_sum_kernel, grid, dim3(kT), 0, st, disp, masks, N, w);
        hipLaunchKernelGGL(ds_mean_kernel, dim3(io_cdiv(n, 64)), dim3(64), 0, st, w, n, nb, value);
    }
    return io_check_launch("instance_depth_select");
}
