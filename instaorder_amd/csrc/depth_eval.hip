// Dense-disparity evaluation on the device: the "median" branch of tools/test_disp_KITTI.py:eval_dense_depth with its
// compute_errors, and the point sampling of tools/test_disp_DIW.py:eval_ordinal_via_disp.  The reference evaluates one
// image at a time and does both on the host in NumPy after a .cpu(); here a whole batch stays on the device.
//
// io_depth_errors_median, six launches per batch whatever B is (grid: blocks-per-image x B):
//   1 stats     per-block min / max of the disparity and count of valid pixels; zeroes the radix histograms
//   2 pass 1    folds the partials (min / max are exact in any order); 11-bit histograms of the top digit of gt and depth
//   3 pass 2    finds each target rank's bucket; 11-bit histograms of the next digit inside it (4 targets)
//   4 pass 3    the same for the last 10 bits
//   5 errors    exact order statistics -> the two medians and the ratio; per-block fp64 sums of the eight errors
//   6 finalize  folds the per-block sums in block order -> one fp64 row per image
// The four targets are the ranks (n-1)/2 and n/2 of gt[valid] and of depth[valid] (NumPy's median: for an even count the
// fp32 mean of the two middle values).  Keys are the fp32 bit patterns mapped to an order-preserving uint32, so the
// selected value is the exact fp32 element.  Histograms are merged with integer atomics (order-independent) and the sums
// go through fixed per-block slabs, so a row depends on its image alone: bitwise the same for every B and every run.
#include "io_common.h"

#include <math.h>

// Elementwise steps round like the reference's fp32 NumPy expressions: plain operators under contract(off) -- the
// __fadd_rn / __fmul_rn wrappers are defined outside this pragma's reach and may still be fused into an fma.
#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / 64;
constexpr int kMaxBlk = 128;      // blocks per image
constexpr int kBins = 2048;
constexpr int kHists = 10;        // per image: pass 1 (gt, depth), pass 2 (4 targets), pass 3 (4 targets)
constexpr int kSums = 8;          // abs_rel, sq_rel, (g-p)^2, d^2, d, a1, a2, a3 with d = log p - log g

int de_blocks(long N) {
    long b = (N + kT * 4 - 1) / (kT * 4);
    return (int)(b < 1 ? 1 : (b > kMaxBlk ? kMaxBlk : b));
}

struct Ws {
    double* sums;      // [B][nb][kSums]
    float* mm;         // [B][nb][2]
    int* cnt;          // [B][nb]
    float* img;        // [B][4]: min, max, ratio
    int* imgn;         // [B]
    unsigned* state;   // [B][2][4][2]: (prefix, rank in bucket) after pass 1 / pass 2
    unsigned* hist;    // [B][kHists][kBins]
};

size_t al(size_t x) { return (x + 255) / 256 * 256; }

size_t ws_layout(int B, int nb, char* base, Ws* w) {
    size_t o = 0;
    const size_t s_sums = al((size_t)B * nb * kSums * 8), s_mm = al((size_t)B * nb * 2 * 4), s_cnt = al((size_t)B * nb * 4),
                 s_img = al((size_t)B * 4 * 4), s_n = al((size_t)B * 4), s_state = al((size_t)B * 16 * 4),
                 s_hist = al((size_t)B * kHists * kBins * 4);
    if (w) {
        w->sums = reinterpret_cast<double*>(base + o);
        w->mm = reinterpret_cast<float*>(base + o + s_sums);
        w->cnt = reinterpret_cast<int*>(base + o + s_sums + s_mm);
        w->img = reinterpret_cast<float*>(base + o + s_sums + s_mm + s_cnt);
        w->imgn = reinterpret_cast<int*>(base + o + s_sums + s_mm + s_cnt + s_img);
        w->state = reinterpret_cast<unsigned*>(base + o + s_sums + s_mm + s_cnt + s_img + s_n);
        w->hist = reinterpret_cast<unsigned*>(base + o + s_sums + s_mm + s_cnt + s_img + s_n + s_state);
    }
    return s_sums + s_mm + s_cnt + s_img + s_n + s_state + s_hist;
}

// order-preserving map of fp32 bit patterns to uint32 (negative values below positive ones) and back
__device__ __forceinline__ unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// gt = float32(raw) / div; valid = min_depth <= gt <= max_depth
__device__ __forceinline__ bool gt_valid(uint16_t raw, float div, float lo, float hi, float& g) {
    g = __fdiv_rn((float)raw, div);
    return lo <= g && g <= hi;
}
// depth = 1 / ((pred - pred.min()) / pred.max() + 1e-3)
__device__ __forceinline__ float to_depth(float p, float mn, float mx) {
    return __fdiv_rn(1.f, __fdiv_rn(p - mn, mx) + 1e-3f);
}

__device__ __forceinline__ float wmin(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wmax(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wsum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wsumd(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Rank k (0-based) among the elements counted by h[nbins] (global): sets out[0] = its bucket, out[1] = its rank inside the
// bucket.  Block-cooperative (all kT threads); 8 (or 4) consecutive bins per thread, one block-wide exclusive scan.
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
    __syncthreads();
}

// ---- launch 1 ----
__global__ __launch_bounds__(kT) void de_stats_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ gt, int N,
                                                      float div, float lo, float hi, Ws w) {
    __shared__ float smn[kWaves], smx[kWaves];
    __shared__ int sc[kWaves];
    const int b = blockIdx.y, nb = gridDim.x;
    const float* p = pred + (size_t)b * N;
    const uint16_t* g = gt + (size_t)b * N;
    float mn = INFINITY, mx = -INFINITY;
    int c = 0;
    for (int i = blockIdx.x * kT + threadIdx.x; i < N; i += nb * kT) {
        const float v = p[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        float gv;
        c += gt_valid(g[i], div, lo, hi, gv);
    }
    unsigned* hs = w.hist + (size_t)b * kHists * kBins;
    for (int i = blockIdx.x * kT + threadIdx.x; i < kHists * kBins; i += nb * kT) hs[i] = 0u;
    mn = wmin(mn); mx = wmax(mx); c = wsum(c);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { smn[wave] = mn; smx[wave] = mx; sc[wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kWaves; ++k) { mn = fminf(mn, smn[k]); mx = fmaxf(mx, smx[k]); c += sc[k]; }
        const size_t o = (size_t)b * nb + blockIdx.x;
        w.mm[o * 2] = mn;
        w.mm[o * 2 + 1] = mx;
        w.cnt[o] = c;
    }
}

// ---- launch 2 ----
__global__ __launch_bounds__(kT) void de_pass1_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ gt, int N,
                                                      float div, float lo, float hi, Ws w) {
    __shared__ unsigned sh[2][kBins];
    __shared__ float sfold[2];
    const int b = blockIdx.y, nb = gridDim.x;
    for (int i = threadIdx.x; i < 2 * kBins; i += kT) (&sh[0][0])[i] = 0u;
    if (threadIdx.x < 64) {          // one wave folds the image's nb <= 128 partials
        float mn = INFINITY, mx = -INFINITY;
        int c = 0;
        for (int j = threadIdx.x; j < nb; j += 64) {
            const size_t o = (size_t)b * nb + j;
            mn = fminf(mn, w.mm[o * 2]);
            mx = fmaxf(mx, w.mm[o * 2 + 1]);
            c += w.cnt[o];
        }
        mn = wmin(mn); mx = wmax(mx); c = wsum(c);
        if (threadIdx.x == 0) {
            sfold[0] = mn;
            sfold[1] = mx;
            if (blockIdx.x == 0) {
                w.img[b * 4] = mn;
                w.img[b * 4 + 1] = mx;
                w.imgn[b] = c;
            }
        }
    }
    __syncthreads();
    const float mn = sfold[0], mx = sfold[1];
    const float* p = pred + (size_t)b * N;
    const uint16_t* g = gt + (size_t)b * N;
    for (int i = blockIdx.x * kT + threadIdx.x; i < N; i += nb * kT) {
        float gv;
        if (gt_valid(g[i], div, lo, hi, gv)) {
            atomicAdd(&sh[0][fkey(gv) >> 21], 1u);
            atomicAdd(&sh[1][fkey(to_depth(p[i], mn, mx)) >> 21], 1u);
        }
    }
    __syncthreads();
    unsigned* hs = w.hist + (size_t)b * kHists * kBins;
    for (int i = threadIdx.x; i < 2 * kBins; i += kT) {
        const unsigned v = (&sh[0][0])[i];
        if (v) atomicAdd(hs + i, v);
    }
}

// target t: 0 / 1 = ranks (n-1)/2, n/2 of gt[valid]; 2 / 3 = the same of depth[valid]
__device__ __forceinline__ unsigned target_rank(int t, int n) { return (t & 1) ? (unsigned)(n / 2) : (unsigned)((n - 1) / 2); }

// ---- launches 3 and 4: q = 1 -> pass-2 histograms (digit bits 20..10), q = 2 -> pass-3 histograms (bits 9..0) ----
__global__ __launch_bounds__(kT) void de_pass_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ gt, int N,
                                                     float div, float lo, float hi, int q, Ws w) {
    __shared__ unsigned sh[4][kBins];
    __shared__ unsigned sel[2], wtot[kWaves], spre[4];
    const int b = blockIdx.y, nb = gridDim.x;
    const int n = w.imgn[b];
    if (n <= 0) return;
    unsigned* hs = w.hist + (size_t)b * kHists * kBins;
    unsigned* st = w.state + (size_t)b * 16;
    for (int t = 0; t < 4; ++t) {
        const unsigned* h = q == 1 ? hs + (t >> 1) * kBins : hs + (2 + t) * kBins;
        const unsigned k = q == 1 ? target_rank(t, n) : st[t * 2 + 1];
        const unsigned pre = q == 1 ? 0u : st[t * 2];
        radix_find(h, kBins, k, sel, wtot);
        if (threadIdx.x == 0) {
            spre[t] = q == 1 ? sel[0] : (pre << 11) | sel[0];
            if (blockIdx.x == 0) {
                st[8 * (q - 1) + t * 2] = spre[t];
                st[8 * (q - 1) + t * 2 + 1] = sel[1];
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < 4 * kBins; i += kT) (&sh[0][0])[i] = 0u;
    __syncthreads();
    const unsigned pre[4] = {spre[0], spre[1], spre[2], spre[3]};
    const int pshift = q == 1 ? 21 : 10, dshift = q == 1 ? 10 : 0;
    const unsigned dmask = q == 1 ? 0x7ffu : 0x3ffu;
    const float mn = w.img[b * 4], mx = w.img[b * 4 + 1];
    const float* p = pred + (size_t)b * N;
    const uint16_t* g = gt + (size_t)b * N;
    for (int i = blockIdx.x * kT + threadIdx.x; i < N; i += nb * kT) {
        float gv;
        if (gt_valid(g[i], div, lo, hi, gv)) {
            const unsigned kg = fkey(gv), kd = fkey(to_depth(p[i], mn, mx));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const unsigned key = t < 2 ? kg : kd;
                if ((key >> pshift) == pre[t]) atomicAdd(&sh[t][(key >> dshift) & dmask], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* dst = hs + (q == 1 ? 2 : 6) * kBins;
    for (int i = threadIdx.x; i < 4 * kBins; i += kT) {
        const unsigned v = (&sh[0][0])[i];
        if (v) atomicAdd(dst + i, v);
    }
}

// ---- launch 5 ----
__global__ __launch_bounds__(kT) void de_errors_kernel(const float* __restrict__ pred, const uint16_t* __restrict__ gt, int N,
                                                       float div, float lo, float hi, Ws w, float* __restrict__ medians) {
    __shared__ unsigned sel[2], wtot[kWaves];
    __shared__ float sval[4];
    __shared__ double sred[kWaves][kSums];
    const int b = blockIdx.y, nb = gridDim.x;
    const int n = w.imgn[b];
    if (n <= 0) {
        if (medians && blockIdx.x == 0 && threadIdx.x == 0) medians[b * 2] = medians[b * 2 + 1] = NAN;
        return;
    }
    const unsigned* hs = w.hist + (size_t)b * kHists * kBins;
    const unsigned* st = w.state + (size_t)b * 16 + 8;
    for (int t = 0; t < 4; ++t) {
        radix_find(hs + (6 + t) * kBins, 1024, st[t * 2 + 1], sel, wtot);
        if (threadIdx.x == 0) sval[t] = fkey_inv((st[t * 2] << 10) | sel[0]);
        __syncthreads();
    }
    // np.median: the middle element, or the fp32 mean of the two middle elements
    const bool odd = n & 1;
    const float med_g = odd ? sval[0] : __fdiv_rn(sval[0] + sval[1], 2.f);
    const float med_d = odd ? sval[2] : __fdiv_rn(sval[2] + sval[3], 2.f);
    const float ratio = __fdiv_rn(med_g, med_d);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        w.img[b * 4 + 2] = ratio;
        if (medians) {
            medians[b * 2] = med_g;
            medians[b * 2 + 1] = med_d;
        }
    }
    const float mn = w.img[b * 4], mx = w.img[b * 4 + 1];
    const float* p = pred + (size_t)b * N;
    const uint16_t* g = gt + (size_t)b * N;
    double acc[kSums];
#pragma unroll
    for (int s = 0; s < kSums; ++s) acc[s] = 0.0;
    for (int i = blockIdx.x * kT + threadIdx.x; i < N; i += nb * kT) {
        float gv;
        if (!gt_valid(g[i], div, lo, hi, gv)) continue;
        float d = to_depth(p[i], mn, mx) * ratio;
        d = d < lo ? lo : d;
        d = d > hi ? hi : d;
        const float thr = fmaxf(__fdiv_rn(gv, d), __fdiv_rn(d, gv));
        const float diff = gv - d;
        const float sq = diff * diff;
        const float ld = (float)log((double)d) - (float)log((double)gv);
        acc[0] += (double)__fdiv_rn(fabsf(diff), gv);
        acc[1] += (double)__fdiv_rn(sq, gv);
        acc[2] += (double)sq;
        acc[3] += (double)(ld * ld);
        acc[4] += (double)ld;
        acc[5] += thr < 1.25f ? 1.0 : 0.0;
        acc[6] += thr < 1.5625f ? 1.0 : 0.0;
        acc[7] += thr < 1.953125f ? 1.0 : 0.0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < kSums; ++s) {
        const double v = wsumd(acc[s]);
        if (lane == 0) sred[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        double v = sred[0][threadIdx.x];
        for (int k = 1; k < kWaves; ++k) v += sred[k][threadIdx.x];
        w.sums[((size_t)b * nb + blockIdx.x) * kSums + threadIdx.x] = v;
    }
}

// ---- launch 6: row = [abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, silog, n_valid, ratio] ----
__global__ __launch_bounds__(64) void de_finalize_kernel(int nb, Ws w, double* __restrict__ out) {
    __shared__ double s[kSums];
    const int b = blockIdx.x;
    const int n = w.imgn[b];
    double* row = out + (size_t)b * 10;
    if (n <= 0) {
        if (threadIdx.x < 10) row[threadIdx.x] = threadIdx.x == 8 ? 0.0 : (double)NAN;
        return;
    }
    if (threadIdx.x < kSums) {
        double v = 0.0;
        for (int k = 0; k < nb; ++k) v += w.sums[((size_t)b * nb + k) * kSums + threadIdx.x];
        s[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double dn = (double)n, md = s[4] / dn;
        row[0] = s[0] / dn;
        row[1] = s[1] / dn;
        row[2] = sqrt(s[2] / dn);
        row[3] = sqrt(s[3] / dn);
        row[4] = s[5] / dn;
        row[5] = s[6] / dn;
        row[6] = s[7] / dn;
        row[7] = sqrt(s[3] / dn - md * md);
        row[8] = dn;
        row[9] = (double)w.img[b * 4 + 2];
    }
}

// ---- io_disp_sample_points ----
// PyTorch's upsample_bilinear2d (align_corners=False, no scale factor) source index and weights along one axis
__device__ __forceinline__ void bl_axis(int in, int out, int d, int& i0, int& i1, float& l0, float& l1) {
    if (in == out) {
        i0 = i1 = d;
        l0 = 1.f;
        l1 = 0.f;
        return;
    }
    const float scale = __fdiv_rn((float)in, (float)out);
    // scale * (d + 0.5) - 0.5 as one fma: what PyTorch's CPU (x86 FMA builds) and CUDA kernels evaluate; the weights are
    // sensitive to it (an ulp of the index is an ulp of the weight times the difference of the taps)
    float r = fmaf(scale, (float)d + 0.5f, -0.5f);
    if (r < 0.f) r = 0.f;
    i0 = min((int)floorf(r), in - 1);
    l1 = fminf(fmaxf(r - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l0 = 1.f - l1;
}

__device__ __forceinline__ float bl_sample(const float* __restrict__ m, int H, int W, int h, int w, int y, int x) {
    y = min(max(y, 0), h - 1);
    x = min(max(x, 0), w - 1);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    bl_axis(H, h, y, y0, y1, hy0, hy1);
    bl_axis(W, w, x, x0, x1, wx0, wx1);
    const float t0 = m[(size_t)y0 * W + x0] * wx0 + m[(size_t)y0 * W + x1] * wx1;
    const float t1 = m[(size_t)y1 * W + x0] * wx0 + m[(size_t)y1 * W + x1] * wx1;
    return t0 * hy0 + t1 * hy1;
}

__global__ __launch_bounds__(kT) void disp_sample_kernel(const float* __restrict__ disp, int B, int H, int W,
                                                         const int* __restrict__ pts, float* __restrict__ vals,
                                                         int* __restrict__ dec) {
    const int b = blockIdx.x * kT + threadIdx.x;
    if (b >= B) return;
    const int* q = pts + (size_t)b * 6;
    const int h = q[0], w = q[1];
    if (h <= 0 || w <= 0) {
        vals[b * 2] = vals[b * 2 + 1] = NAN;
        dec[b] = 0;
        return;
    }
    const float* m = disp + (size_t)b * H * W;
    const float a = bl_sample(m, H, W, h, w, q[2], q[3]), c = bl_sample(m, H, W, h, w, q[4], q[5]);
    vals[b * 2] = a;
    vals[b * 2 + 1] = c;
    // disparity order is the opposite of depth order (test_disp_DIW.py:136-142)
    dec[b] = a > c ? '<' : (a < c ? '>' : (a == c ? '=' : 0));
}

}  // namespace

extern "C" size_t io_depth_errors_median_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(B, de_blocks((long)H * W), nullptr, nullptr);
}

extern "C" int io_depth_errors_median(const float* pred, const uint16_t* gt, int B, int H, int W, float gt_div,
                                      float min_depth, float max_depth, double* out, float* medians,
                                      void* workspace, size_t workspace_bytes, hipStream_t st) {
    IO_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 30), IO_ERR_SHAPE,
               "depth_errors_median: B=%d H=%d W=%d", B, H, W);
    IO_REQUIRE(pred && gt && out, IO_ERR_SHAPE, "depth_errors_median: null pointer");
    IO_REQUIRE(gt_div > 0.f && min_depth > 0.f && max_depth >= min_depth, IO_ERR_SHAPE,
               "depth_errors_median: gt_div=%g min_depth=%g max_depth=%g", gt_div, min_depth, max_depth);
    IO_REQUIRE(workspace && workspace_bytes >= io_depth_errors_median_workspace_bytes(B, H, W), IO_ERR_WORKSPACE,
               "depth_errors_median: workspace too small");
    const int N = H * W, nb = de_blocks(N);
    Ws w;
    ws_layout(B, nb, static_cast<char*>(workspace), &w);
    const dim3 grid(nb, B);
    hipLaunchKernelGGL(de_stats_kernel, grid, dim3(kT), 0, st, pred, gt, N, gt_div, min_depth, max_depth, w);
    hipLaunchKernelGGL(de_pass1_kernel, grid, dim3(kT), 0, st, pred, gt, N, gt_div, min_depth, max_depth, w);
    hipLaunchKernelGGL(de_pass_kernel, grid, dim3(kT), 0, st, pred, gt, N, gt_div, min_depth, max_depth, 1, w);
    hipLaunchKernelGGL(de_pass_kernel, grid, dim3(kT), 0, st, pred, gt, N, gt_div, min_depth, max_depth, 2, w);
    hipLaunchKernelGGL(de_errors_kernel, grid, dim3(kT), 0, st, pred, gt, N, gt_div, min_depth, max_depth, w, medians);
    hipLaunchKernelGGL(de_finalize_kernel, dim3(B), dim3(64), 0, st, nb, w, out);
    return io_check_launch("depth_errors_median");
}

extern "C" int io_disp_sample_points(const float* disp, int B, int H, int W, const int* points, float* values, int* decisions,
                                     hipStream_t st) {
    IO_REQUIRE(B > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), IO_ERR_SHAPE, "disp_sample_points: B=%d H=%d W=%d", B,
               H, W);
    IO_REQUIRE(disp && points && values && decisions, IO_ERR_SHAPE, "disp_sample_points: null pointer");
    hipLaunchKernelGGL(disp_sample_kernel, dim3(io_cdiv(B, kT)), dim3(kT), 0, st, disp, B, H, W, points, values, decisions);
    return io_check_launch("disp_sample_points");
}
