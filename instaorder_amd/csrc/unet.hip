// PCNet-M (UNet) kernels, NHWC fp32.  Training adds the backward of the three UNet-only operators (the convolutions and
// BatchNorms of a training step are the dense launchers'): io_maxpool2x2_bwd, io_up2x_concat_bwd, io_unet_head_bwd -- one pass
// over each tensor in 16-byte accesses, no floating-point atomics, every sum in a fixed order.  Inference: what the
// eval-mode forward of instaorder_amd/unet.py needs beyond the dense convolution launcher (io_conv2d_fwd_bias_dt:
// Co % 64 == 0, Ci % 32 == 0):
//   io_conv3x3_co32_fwd  3x3 / stride 1 / pad 1 convolution with 32 output channels, + bias (+ ReLU)
//   io_maxpool2x2_fwd    nn.MaxPool2d(2)
//   io_up2x_concat_fwd   cat([x2, bilinear x2 (align_corners) of x1], channel) in one pass
//   io_unet_pack_input   the two mask planes of a patch -> the packed network input (erase + category folded in)
//   io_unet_head         1x1 outc + softmax threshold + per-patch completion count (+ logits, + the two CE sums)
//
// The 32-channel convolution.  One 32-wide N tile is the whole output, so a block owns a 16-row x 32-column patch of one
// sample's output and each of its 4 waves owns 4 of those rows: 4 independent 32 x 32 accumulators per wave, which is what
// v_mfma_f32_32x32x2_f32 (64 cycles issue, 64 cycles dependent) needs to run back to back.  K = 9 taps x Ci is walked in
// chunks of KC input channels; per chunk the block stages the 18 x 34 input halo ONCE (channel-major planes, so the 9 taps
// read shifted windows of the same plane) and the chunk's [9][KC][32] filter slice.  Per (tap, channel pair) a wave reads
// one B fragment and 4 A fragments for 4 MFMAs = 256 matrix cycles: the LDS pipe is nearly idle, and with 60 KB per block
// two blocks share a CU, one loading while the other multiplies.
//   A fragment: lane (i = lane & 31, k = lane >> 5) reads plane[c + k][row][x + i]: 32 consecutive words per k, the two k
// a plane apart; kPlane % 64 == 32 puts the halves on disjoint banks.  B fragment: wt[tap][c + k][i]: 64 consecutive words.
//   Staging stores: a wave holds 64 / (KC / 4) consecutive pixels for each of its KC / 4 channel quads and writes one
// component at a time, i.e. to planes 4 apart -- 4 * kPlane == 0 (mod 64), all quads on the same banks.  So every group of
// 4 planes is skewed by 64 / (KC / 4) words (plane_off): the quads land on disjoint bank windows, and planes c, c + 1 of a
// fragment read stay in one group, 32 (mod 64) apart.
#include <math.h>
#include <stdlib.h>

#include "io_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileR = 16, kTileC = 32;                   // output rows / columns of a block
constexpr int kHaloR = kTileR + 2, kHaloC = kTileC + 2;
constexpr int kPlane = 672;                               // >= kHaloR * kHaloC = 612, and == 32 (mod 64)
static_assert(kPlane >= kHaloR * kHaloC && kPlane % 64 == 32, "plane stride");
template <int KC> __device__ __host__ constexpr int plane_off(int p) { return p * kPlane + (64 / (KC / 4)) * (p >> 2); }
template <int KC> constexpr int in_floats() { return plane_off<KC>(KC - 1) + kPlane; }      // a multiple of 4

std::atomic<int> g_co32{-1};     // the route switch of unet.py (io_set_unet_co32); -1 = not read from the environment yet

template <int KC>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_co32_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                                   const float* __restrict__ bias, float* __restrict__ y,
                                                                   int H, int W, int Ci, int relu, int tiles_x, int tiles_y) {
    extern __shared__ float smem[];
    float* in_s = smem;                       // plane p at plane_off<KC>(p)
    float* wt_s = smem + in_floats<KC>();     // [9][KC][32]
    int t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, n = t / tiles_y;
    const int y0 = ty * kTileR, x0 = tx * kTileC;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int li = lane & 31, lk = lane >> 5;
    const bool live = y0 + 4 * wv < H;        // wave-uniform: a wave whose rows all lie below the map only keeps the barriers

    f32x16 acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;

    const float* xn = x + (size_t)n * H * W * Ci;
    for (int c0 = 0; c0 < Ci; c0 += KC) {
        if (c0) __syncthreads();              // the previous chunk's fragments have been read
        for (int idx = threadIdx.x; idx < kHaloR * kHaloC * (KC / 4); idx += kThreads) {
            const int c4 = idx % (KC / 4), pix = idx / (KC / 4);
            const int r = pix / kHaloC, cx = pix - r * kHaloC;
            const int gy = y0 - 1 + r, gx = x0 - 1 + cx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = io_ldv(xn + ((size_t)gy * W + gx) * Ci + c0 + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) in_s[plane_off<KC>(4 * c4 + e) + pix] = v[e];
        }
        for (int idx = threadIdx.x; idx < 9 * KC * 8; idx += kThreads) {
            const int tap = idx / (KC * 8), rem = idx - tap * (KC * 8);
            io_stv(wt_s + tap * KC * 32 + rem * 4, io_ldv(wp + ((size_t)tap * Ci + c0) * 32 + rem * 4));
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3, dx = tap % 3;
                const float* ap = in_s + lk * kPlane + (4 * wv + dy) * kHaloC + dx + li;      // (lk does not change the group)
                const float* bp = wt_s + (tap * KC + lk) * 32 + li;
#pragma unroll
                for (int kk = 0; kk < KC / 2; ++kk) {
                    const float b = bp[kk * 2 * 32];
                    constexpr int kSkew = 64 / (KC / 4);
                    const float* aq = ap + kk * 2 * kPlane + kSkew * (kk >> 1);               // = plane_off<KC>(2 kk + lk)
                    const float a0 = aq[0], a1 = aq[kHaloC], a2 = aq[2 * kHaloC], a3 = aq[3 * kHaloC];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b, acc[3], 0, 0, 0);
                }
            }
        }
    }
    if (!live) return;
    // C / D map of the 32 x 32 forms: column (output channel) = lane & 31, row (pixel) = 8 (e >> 2) + 4 (lane >> 5) + (e & 3)
    const float bo = bias[li];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gy = y0 + 4 * wv + r;
        if (gy >= H) break;
        float* yr = y + (((size_t)n * H + gy) * W) * 32 + li;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int gx = x0 + 8 * (e >> 2) + 4 * lk + (e & 3);
            if (gx < W) {
                float v = acc[r][e] + bo;
                if (relu) v = v > 0.f ? v : 0.f;
                yr[(size_t)gx * 32] = v;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void maxpool2x2_kernel(const float* __restrict__ x, int H, int W, int C4, size_t total,
                                                              float* __restrict__ out) {
    const int OW = W / 2, OH = H / 2;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int q = (int)(i % C4);
        size_t p = i / C4;
        const int ow = (int)(p % OW);
        p /= OW;
        const int oh = (int)(p % OH);
        const size_t n = p / OH;
        const float* s = x + (((n * H + 2 * oh) * W + 2 * ow) * C4 + q) * 4;
        const f32x4 a = io_ldv(s), b = io_ldv(s + (size_t)C4 * 4), c = io_ldv(s + (size_t)W * C4 * 4),
                    d = io_ldv(s + ((size_t)W + 1) * C4 * 4);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
        io_stv(out + i * 4, r);
    }
}

// source index and weights of nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True): dst * (h - 1) / (2h - 1)
struct Lerp {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Lerp lerp_aligned(int dst, int h) {
    const float sc = h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.f;
    const float src = sc * (float)dst;
    Lerp l;
    l.i0 = (int)src;
    if (l.i0 > h - 1) l.i0 = h - 1;
    l.i1 = l.i0 + (l.i0 < h - 1 ? 1 : 0);
    l.w1 = src - (float)l.i0;
    l.w0 = 1.f - l.w1;
    return l;
}

// one output row per blockIdx.y step; a thread moves 4 channels of the concatenated pixel
__global__ __launch_bounds__(kThreads) void up2x_concat_kernel(const float* __restrict__ x2, const float* __restrict__ x1,
                                                               int N, int h, int w, int C2q, int C1q,
                                                               float* __restrict__ out) {
    const int OH = 2 * h, OW = 2 * w, Cq = C2q + C1q, rowlen = OW * Cq;
    for (int row = blockIdx.y; row < N * OH; row += gridDim.y) {
        const int n = row / OH, oh = row - n * OH;
        const Lerp lh = lerp_aligned(oh, h);
        const float* r0 = x1 + ((size_t)n * h + lh.i0) * w * C1q * 4;
        const float* r1 = x1 + ((size_t)n * h + lh.i1) * w * C1q * 4;
        const float* s2 = x2 + (size_t)row * OW * C2q * 4;
        float* o = out + (size_t)row * rowlen * 4;
        for (int j = blockIdx.x * kThreads + threadIdx.x; j < rowlen; j += gridDim.x * kThreads) {
            const int ow = j / Cq, q = j - ow * Cq;
            f32x4 r;
            if (q < C2q) {
                r = io_ldv(s2 + ((size_t)ow * C2q + q) * 4);
            } else {
                const Lerp lw = lerp_aligned(ow, w);
                const int qq = q - C2q;
                const f32x4 a = io_ldv(r0 + ((size_t)lw.i0 * C1q + qq) * 4), b = io_ldv(r0 + ((size_t)lw.i1 * C1q + qq) * 4);
                const f32x4 c = io_ldv(r1 + ((size_t)lw.i0 * C1q + qq) * 4), d = io_ldv(r1 + ((size_t)lw.i1 * C1q + qq) * 4);
                // same association as PyTorch's CPU kernel (and io_upsample2x_bilinear_fwd)
                r = lh.w0 * (lw.w0 * a + lw.w1 * b) + lh.w1 * (lw.w0 * c + lw.w1 * d);
            }
            io_stv(o + (size_t)j * 4, r);
        }
    }
}

// out[p][pix][0] = (erase && m2 == 1 ? 0 : m1) * scale[p], out[p][pix][1] = m2, the other stored channels 0
__global__ __launch_bounds__(kThreads) void unet_pack_input_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                                   const float* __restrict__ scale, int HW, size_t total,
                                                                   int Cs, int erase, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const float e = m2[i];
        float a = m1[i];
        if (erase && e == 1.f) a = 0.f;
        if (scale) a *= scale[i / HW];
        float* o = out + i * Cs;
        io_stv(o, f32x4{a, e, 0.f, 0.f});
        for (int c = 4; c < Cs; c += 4) io_stv(o + c, f32x4{0.f, 0.f, 0.f, 0.f});
    }
}

// One thread per pixel: the two logits, the thresholded completion, the pixel's vote for the patch count, and in loss mode
// its cross-entropy term on the inside / outside sum.  Counts are integer atomics (exact in any order); the CE sums are
// per-block partials in block order, added up by unet_loss_reduce_kernel in a fixed tree.
__global__ __launch_bounds__(kThreads) void unet_head_kernel(const float* __restrict__ act, const float* __restrict__ wo,
                                                             const float* __restrict__ bo, const float* __restrict__ m1,
                                                             const float* __restrict__ m2, const uint8_t* __restrict__ target,
                                                             int HW, int Cs, float logit_th, uint8_t* __restrict__ comp,
                                                             int* __restrict__ counts, float* __restrict__ logits,
                                                             float* __restrict__ partials) {
    __shared__ float red[2][kThreads / 64];
    const int p = blockIdx.y;
    const int pix = blockIdx.x * kThreads + threadIdx.x;
    const bool on = pix < HW;
    bool vote = false;
    float ce_in = 0.f, ce_out = 0.f;
    if (on) {
        const size_t g = (size_t)p * HW + pix;
        const float* a = act + g * Cs;
        float l0 = 0.f, l1 = 0.f;
        for (int c = 0; c < Cs; c += 4) {
            const f32x4 v = io_ldv(a + c), w0 = io_ldv(wo + c), w1 = io_ldv(wo + Cs + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                l0 = fmaf(v[e], w0[e], l0);
                l1 = fmaf(v[e], w1[e], l1);
            }
        }
        l0 += bo[0];
        l1 += bo[1];
        if (logits) {
            logits[2 * g] = l0;
            logits[2 * g + 1] = l1;
        }
        const float er = m2[g];
        const float vis = er == 1.f ? 0.f : m1[g];           // the erased target patch
        const bool c1 = (l1 - l0) > logit_th;                 // softmax(l)[1] > th
        if (comp) comp[g] = c1 ? 1 : 0;
        vote = ((c1 ? 1.f : 0.f) > vis) && er == 1.f;
        if (partials) {
            const float mx = fmaxf(l0, l1);
            const float lse = mx + logf(expf(l0 - mx) + expf(l1 - mx));
            const float ce = lse - (target[g] ? l1 : l0);
            if (er != 0.f) ce_in = ce; else ce_out = ce;
        }
    }
    const unsigned long long b = __ballot(vote);
    if (counts && (threadIdx.x & 63) == 0 && b) atomicAdd(counts + p, __popcll(b));
    if (partials) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            ce_in += __shfl_xor(ce_in, s);
            ce_out += __shfl_xor(ce_out, s);
        }
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = ce_in;
            red[1][threadIdx.x >> 6] = ce_out;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const float* r = red[threadIdx.x];
            partials[2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
        }
    }
}

// sums[0] = inside, sums[1] = outside: one block, thread t adds partials t, t + 256, ... in fp64, then a fixed tree
__global__ __launch_bounds__(kThreads) void unet_loss_reduce_kernel(const float* __restrict__ partials, int nblocks,
                                                                    float* __restrict__ sums) {
    __shared__ double red[2][kThreads];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) {
        a += (double)partials[2 * i];
        b += (double)partials[2 * i + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) sums[threadIdx.x] = (float)red[threadIdx.x][0];
}

// ---- training: the backward of the three UNet-only operators -------------------------------------------------------------
// Backward of nn.MaxPool2d(2): a thread owns 4 channels of one 2x2 window.  The gradient goes to the FIRST maximum in (row,
// column) order (PyTorch's rule: a later element replaces the running maximum only when strictly greater), the other three
// positions get 0; ``add`` (shaped like dx, may BE dx: every element is read by the thread that then writes it) is summed in.
__global__ __launch_bounds__(kThreads) void maxpool2x2_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                  const float* add, int H, int W, int C4, size_t total,
                                                                  float* dx) {
    const int OW = W / 2, OH = H / 2;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int q = (int)(i % C4);
        size_t p = i / C4;
        const int ow = (int)(p % OW);
        p /= OW;
        const int oh = (int)(p % OH);
        const size_t n = p / OH;
        const size_t o00 = (((n * H + 2 * oh) * W + 2 * ow) * C4 + q) * 4;
        const size_t off[4] = {o00, o00 + (size_t)C4 * 4, o00 + (size_t)W * C4 * 4, o00 + ((size_t)W + 1) * C4 * 4};
        const f32x4 g = io_ldv(dy + i * 4);
        f32x4 v[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = io_ldv(x + off[k]);
            r[k] = add ? io_ldv(add + off[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = v[0][e];
            int at = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][e] > m) {
                    m = v[k][e];
                    at = k;
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k][e] += (at == k) ? g[e] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) io_stv(dx + off[k], r[k]);
    }
}

// dx2 = the first C2 channels of dcat: a thread moves 4 channels of one pixel
__global__ __launch_bounds__(kThreads) void concat_split_kernel(const float* __restrict__ dcat, int C2q, int Cq, size_t total,
                                                                float* __restrict__ dx2) {
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const size_t pix = i / C2q;
        const int q = (int)(i - pix * C2q);
        io_stv(dx2 + i * 4, io_ldv(dcat + (pix * Cq + q) * 4));
    }
}

// The weight with which destination index ``dst`` of the x2 interpolation reads source index ``src`` (0: it does not): the
// forward's own lerp_aligned, so the transpose uses the weights the forward used.  A destination at the clamped edge reads
// one source twice (i0 == i1): both weights count.
__device__ __forceinline__ float lerp_weight_of(int dst, int h, int src) {
    const Lerp l = lerp_aligned(dst, h);
    return (l.i0 == src ? l.w0 : 0.f) + (l.i1 == src ? l.w1 : 0.f);
}

// dx1 = transpose of the interpolation, in gather form: a thread owns 4 channels of one SOURCE pixel and sums, in (row,
// column) order, what the destination pixels that read it contribute.  A source index s is read by destinations within
// [2 s - 2, 2 s + 2] (the scale (h - 1) / (2 h - 1) lies in [1/3, 1/2)); the window below has one more on the right for the
// rounding of the forward's fp32 index, and a destination outside the support simply has weight 0.
constexpr int kUpWin = 6;
__global__ __launch_bounds__(kThreads) void up2x_bwd_kernel(const float* __restrict__ dcat, int h, int w, int C2q, int C1q,
                                                            size_t total, float* __restrict__ dx1) {
    const int Cq = C2q + C1q, OH = 2 * h, OW = 2 * w;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int q = (int)(i % C1q);
        size_t p = i / C1q;
        const int sx = (int)(p % w);
        p /= w;
        const int sy = (int)(p % h);
        const size_t n = p / h;
        float wy[kUpWin], wx[kUpWin];
#pragma unroll
        for (int k = 0; k < kUpWin; ++k) {
            const int oy = 2 * sy - 2 + k, ox = 2 * sx - 2 + k;
            wy[k] = (oy >= 0 && oy < OH) ? lerp_weight_of(oy, h, sy) : 0.f;
            wx[k] = (ox >= 0 && ox < OW) ? lerp_weight_of(ox, w, sx) : 0.f;
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < kUpWin; ++ky) {
            if (wy[ky] == 0.f) continue;
            const float* row = dcat + ((n * OH + (size_t)(2 * sy - 2 + ky)) * OW * Cq + C2q + q) * 4;
#pragma unroll
            for (int kx = 0; kx < kUpWin; ++kx) {
                if (wx[kx] == 0.f) continue;
                acc += (wy[ky] * wx[kx]) * io_ldv(row + (size_t)(2 * sx - 2 + kx) * Cq * 4);
            }
        }
        io_stv(dx1 + i * 4, acc);
    }
}

// Backward of the 1x1 head under MaskWeightedCrossEntropyLoss, one pass over the last activation x[pixels][64].  A block owns
// 256 consecutive pixels; 16 neighbouring lanes own one pixel (lane q of the group: channels 4 q .. 4 q + 3), so every load of x
// and every store of dx is a contiguous 256-byte row.  Per pixel: the two logits (16-lane butterfly: every lane ends with
// the same bits), dlogit_c = wgt (softmax_c - [c == target]) scale, dx = dlogit . wo, and the lane's share of dwo; lane 0 of
// the group also keeps dbo and the pixel's cross-entropy term.  Block partials [128 dwo | 2 dbo | 2 CE sums] are written in
// block order and added by unet_head_bwd_reduce_kernel in a fixed order: no atomics, two runs give the same bits.
constexpr int kHeadCs = 64, kHeadCols = 2 * kHeadCs + 4;
__global__ __launch_bounds__(kThreads) void unet_head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ wo,
                                                                 const float* __restrict__ bo, const uint8_t* __restrict__ target,
                                                                 const float* __restrict__ eraser, size_t total,
                                                                 float inmask_weight, float scale, const float* __restrict__ gscale,
                                                                 float* __restrict__ dx, float* __restrict__ partials) {
    __shared__ float red[kThreads / 64][kHeadCols];
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const f32x4 w0 = io_ldv(wo + 4 * q), w1 = io_ldv(wo + kHeadCs + 4 * q);
    const float b0 = bo[0], b1 = bo[1];
    const float sc = gscale ? scale * gscale[0] : scale;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    float s4[4] = {0.f, 0.f, 0.f, 0.f};                 // dbo[0], dbo[1], CE inside, CE outside (lane 0 of a group only)
    const size_t base = (size_t)blockIdx.x * kThreads;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const size_t pix = base + it * 16 + g;
        const bool on = pix < total;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (on) v = io_ldv(x + pix * kHeadCs + 4 * q);
        float l0 = 0.f, l1 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            l0 = fmaf(v[e], w0[e], l0);
            l1 = fmaf(v[e], w1[e], l1);
        }
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1) {
            l0 += __shfl_xor(l0, s);
            l1 += __shfl_xor(l1, s);
        }
        if (on) {
            l0 += b0;
            l1 += b1;
            const float er = eraser[pix];
            const bool t1 = target[pix] != 0;
            const float mx = fmaxf(l0, l1);
            const float e0 = expf(l0 - mx), e1 = expf(l1 - mx), se = e0 + e1;
            const float wgt = (er != 0.f ? inmask_weight : 1.f) * sc;
            const float d0 = wgt * (e0 / se - (t1 ? 0.f : 1.f)), d1 = wgt * (e1 / se - (t1 ? 1.f : 0.f));
            io_stv(dx + pix * kHeadCs + 4 * q, d0 * w0 + d1 * w1);
            a0 += d0 * v;
            a1 += d1 * v;
            if (q == 0) {
                const float ce = mx + logf(se) - (t1 ? l1 : l0);
                s4[0] += d0;
                s4[1] += d1;
                if (er != 0.f) s4[2] += ce; else s4[3] += ce;
            }
        }
    }
    // the 4 groups of a wave (lanes q, q + 16, q + 32, q + 48), then the 4 waves through LDS
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a0[e] += __shfl_xor(a0[e], s);
            a1[e] += __shfl_xor(a1[e], s);
        }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) s4[e] += __shfl_xor(s4[e], s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane < 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[wv][4 * lane + e] = a0[e];
            red[wv][kHeadCs + 4 * lane + e] = a1[e];
        }
    }
    if (lane == 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wv][2 * kHeadCs + e] = s4[e];
    __syncthreads();
    if ((int)threadIdx.x < kHeadCols) {
        const int c = threadIdx.x;
        partials[(size_t)blockIdx.x * kHeadCols + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// column c of the block partials -> dwo (c < 128), dbo (128, 129), the CE sums (130, 131; optional): block c, thread t adds
// partials t, t + 256, ... in fp64, then a fixed tree
__global__ __launch_bounds__(kThreads) void unet_head_bwd_reduce_kernel(const float* __restrict__ partials, int nblocks,
                                                                        float* __restrict__ dwo, float* __restrict__ dbo,
                                                                        float* __restrict__ sums) {
    __shared__ double red[kThreads];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) a += (double)partials[(size_t)i * kHeadCols + c];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float v = (float)red[0];
        if (c < 2 * kHeadCs) dwo[c] = v;
        else if (c < 2 * kHeadCs + 2) dbo[c - 2 * kHeadCs] = v;
        else if (sums) sums[c - 2 * kHeadCs - 2] = v;
    }
}

unsigned ew_grid(size_t total) {
    const size_t b = (total + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

template <int KC> int launch_co32(const float* x, const float* wp, const float* bias, float* y, int N, int H, int W, int Ci,
                                  int relu, hipStream_t st) {
    static std::atomic<unsigned long long> once{0};
    const size_t lds = (size_t)(in_floats<KC>() + 9 * KC * 32) * sizeof(float);
    if (io_first_on_device(once) && lds > 48 * 1024) {
        if (hipFuncSetAttribute((const void*)conv3x3_co32_kernel<KC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
            (void)hipGetLastError();
            io_set_error("conv3x3_co32: cannot reserve %zu bytes of LDS", lds);
            return IO_ERR_LAUNCH;
        }
    }
    const int tiles_x = io_cdiv(W, kTileC), tiles_y = io_cdiv(H, kTileR);
    const long tiles = (long)N * tiles_x * tiles_y;
    IO_REQUIRE(tiles < (1L << 31), IO_ERR_SHAPE, "conv3x3_co32: grid too large");
    hipLaunchKernelGGL(conv3x3_co32_kernel<KC>, dim3((unsigned)tiles), dim3(kThreads), lds, st, x, wp, bias, y, H, W, Ci, relu,
                       tiles_x, tiles_y);
    return io_check_launch("conv3x3_co32");
}

}  // namespace

extern "C" int io_get_unet_co32(void) {
    int v = g_co32.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* e = getenv("IO_UNET_CO32");
        v = (e && e[0] == '0') ? 0 : 1;
        g_co32.store(v, std::memory_order_relaxed);
    }
    return v;
}
extern "C" int io_set_unet_co32(int on) {
    const int prev = io_get_unet_co32();
    g_co32.store(on ? 1 : 0, std::memory_order_relaxed);
    return prev;
}

extern "C" int io_conv3x3_co32_fwd(const float* x, const float* wp, const float* bias, float* y, int N, int H, int W, int Cin,
                                   int Cout, int relu, hipStream_t st) {
    IO_REQUIRE(x && wp && bias && y, IO_ERR_SHAPE, "conv3x3_co32: input, filter, bias and output are required");
    IO_REQUIRE(Cout == 32, IO_ERR_SHAPE, "conv3x3_co32: Cout=%d, the kernel writes exactly 32 output channels", Cout);
    IO_REQUIRE(Cin == 8 || Cin == 32 || Cin == 64 || Cin == 128, IO_ERR_SHAPE,
               "conv3x3_co32: Cin=%d must be 8 (packed), 32, 64 or 128", Cin);
    IO_REQUIRE(N > 0 && H > 0 && W > 0 && (double)N * H * W < 2.0e9, IO_ERR_SHAPE, "conv3x3_co32: N=%d H=%d W=%d", N, H, W);
    const double px = (double)N * H * W;
    IoProfScope prof(IO_PROF_UNET_CO32, 2.0 * px * 9 * Cin * 32, 4.0 * px * (Cin + 32), st);
    if (Cin == 8) return launch_co32<8>(x, wp, bias, y, N, H, W, Cin, relu, st);
    return launch_co32<16>(x, wp, bias, y, N, H, W, Cin, relu, st);
}

extern "C" int io_maxpool2x2_fwd(const float* x, int N, int H, int W, int C, float* out, hipStream_t st) {
    IO_REQUIRE(x && out && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, IO_ERR_SHAPE, "maxpool2x2: N=%d H=%d W=%d C=%d (C %% 4)",
               N, H, W, C);
    IO_REQUIRE(H % 2 == 0 && W % 2 == 0, IO_ERR_SHAPE, "maxpool2x2: H=%d and W=%d must be even", H, W);
    const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
    IoProfScope prof(IO_PROF_UNET, 0.0, 5.0 * 4 * total * 4, st);
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3(ew_grid(total)), dim3(kThreads), 0, st, x, H, W, C / 4, total, out);
    return io_check_launch("maxpool2x2");
}

extern "C" int io_up2x_concat_fwd(const float* x2, const float* x1, int N, int h, int w, int C2, int C1, float* out,
                                  hipStream_t st) {
    IO_REQUIRE(x2 && x1 && out && N > 0 && h > 0 && w > 0 && C1 > 0 && C2 > 0 && C1 % 4 == 0 && C2 % 4 == 0, IO_ERR_SHAPE,
               "up2x_concat: N=%d h=%d w=%d C2=%d C1=%d (channel counts are multiples of 4)", N, h, w, C2, C1);
    IO_REQUIRE((double)N * h * 2 < 2.0e9 && (double)w * 2 * (C1 + C2) < 2.0e9, IO_ERR_SHAPE, "up2x_concat: tensor too large");
    const long rowlen = (long)2 * w * ((C1 + C2) / 4), rows = (long)N * 2 * h;
    const long gx = (rowlen + kThreads - 1) / kThreads;
    IoProfScope prof(IO_PROF_UNET, 0.0, 4.0 * rows * 2 * w * (2.0 * C2 + 1.25 * C1), st);
    hipLaunchKernelGGL(up2x_concat_kernel, dim3((unsigned)(gx > 64 ? 64 : gx), (unsigned)(rows > 65535 ? 65535 : rows)),
                       dim3(kThreads), 0, st, x2, x1, N, h, w, C2 / 4, C1 / 4, out);
    return io_check_launch("up2x_concat");
}

extern "C" int io_unet_pack_input(const float* m1, const float* m2, const float* scale, int P, int HW, int Cs, int erase,
                                  float* out, hipStream_t st) {
    IO_REQUIRE(m1 && m2 && out && P > 0 && HW > 0 && Cs >= 4 && Cs % 4 == 0, IO_ERR_SHAPE, "unet_pack_input: P=%d HW=%d Cs=%d", P,
               HW, Cs);
    const size_t total = (size_t)P * HW;
    IoProfScope prof(IO_PROF_UNET, 0.0, 4.0 * total * (2 + Cs), st);
    hipLaunchKernelGGL(unet_pack_input_kernel, dim3(ew_grid(total)), dim3(kThreads), 0, st, m1, m2, scale, HW, total, Cs, erase,
                       out);
    return io_check_launch("unet_pack_input");
}

extern "C" size_t io_unet_head_partial_floats(int P, int HW) {
    if (P <= 0 || HW <= 0) return 0;
    return 2 * (size_t)P * ((HW + kThreads - 1) / kThreads);
}

extern "C" int io_unet_head(const float* act, const float* wo, const float* bo, const float* m1, const float* m2,
                            const uint8_t* target, int P, int HW, int Cs, float th, uint8_t* comp, int32_t* counts,
                            float* logits, float* partials, size_t partial_floats, float* loss_sums, hipStream_t st) {
    IO_REQUIRE(act && wo && bo && m1 && m2 && P > 0 && P <= 65535 && HW > 0 && Cs >= 4 && Cs % 4 == 0, IO_ERR_SHAPE,
               "unet_head: P=%d (1..65535) HW=%d Cs=%d (a multiple of 4)", P, HW, Cs);
    IO_REQUIRE(th > 0.f && th < 1.f, IO_ERR_SHAPE, "unet_head: th=%g must lie inside (0, 1)", (double)th);
    IO_REQUIRE((target != nullptr) == (loss_sums != nullptr) && (target != nullptr) == (partials != nullptr), IO_ERR_SHAPE,
               "unet_head: the loss mode takes target, partials and loss_sums together");
    const int bx = (HW + kThreads - 1) / kThreads;
    IO_REQUIRE(!partials || partial_floats >= io_unet_head_partial_floats(P, HW), IO_ERR_WORKSPACE,
               "unet_head: partials %zu < %zu floats", partial_floats, io_unet_head_partial_floats(P, HW));
    IO_REQUIRE((double)P * bx < 2.0e9, IO_ERR_SHAPE, "unet_head: too many blocks");
    IoProfScope prof(IO_PROF_UNET, 4.0 * P * HW * Cs, 4.0 * P * HW * (Cs + 2), st);
    if (counts && hipMemsetAsync(counts, 0, sizeof(int32_t) * P, st) != hipSuccess) return io_check_launch("unet_head(memset)");
    // softmax(l)[1] > th  <=>  l1 - l0 > ln(th / (1 - th))
    const float logit_th = (float)log((double)th / (1.0 - (double)th));
    hipLaunchKernelGGL(unet_head_kernel, dim3(bx, P), dim3(kThreads), 0, st, act, wo, bo, m1, m2, target, HW, Cs, logit_th, comp,
                       counts, logits, partials);
    int rc = io_check_launch("unet_head");
    if (rc || !partials) return rc;
    hipLaunchKernelGGL(unet_loss_reduce_kernel, dim3(1), dim3(kThreads), 0, st, partials, P * bx, loss_sums);
    return io_check_launch("unet_loss_reduce");
}

// ---- training (the backward launches of ops.max_pool_2x2 / ops.up2x_concat / ops.unet_head_loss) ---------------------------
extern "C" int io_maxpool2x2_bwd(const float* dy, const float* x, const float* add, int N, int H, int W, int C, float* dx,
                                 hipStream_t st) {
    IO_REQUIRE(dy && x && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, IO_ERR_SHAPE,
               "maxpool2x2_bwd: N=%d H=%d W=%d C=%d (C %% 4)", N, H, W, C);
    IO_REQUIRE(H % 2 == 0 && W % 2 == 0, IO_ERR_SHAPE, "maxpool2x2_bwd: H=%d and W=%d must be even", H, W);
    const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
    IoProfScope prof(IO_PROF_UNET, 0.0, 4.0 * total * 4 * (add ? 13.0 : 9.0), st);
    hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(ew_grid(total)), dim3(kThreads), 0, st, dy, x, add, H, W, C / 4, total, dx);
    return io_check_launch("maxpool2x2_bwd");
}

extern "C" int io_up2x_concat_bwd(const float* dcat, int N, int h, int w, int C2, int C1, float* dx2, float* dx1,
                                  hipStream_t st) {
    IO_REQUIRE(dcat && dx2 && dx1 && N > 0 && h > 0 && w > 0 && C1 > 0 && C2 > 0 && C1 % 4 == 0 && C2 % 4 == 0, IO_ERR_SHAPE,
               "up2x_concat_bwd: N=%d h=%d w=%d C2=%d C1=%d (channel counts are multiples of 4)", N, h, w, C2, C1);
    IO_REQUIRE((double)N * h * 2 < 2.0e9 && (double)w * 2 * (C1 + C2) < 2.0e9, IO_ERR_SHAPE, "up2x_concat_bwd: tensor too large");
    const size_t t2 = (size_t)N * 2 * h * 2 * w * (C2 / 4), t1 = (size_t)N * h * w * (C1 / 4);
    IoProfScope prof(IO_PROF_UNET, 0.0, 4.0 * (2.0 * t2 * 4 + 5.0 * t1 * 4), st);
    hipLaunchKernelGGL(concat_split_kernel, dim3(ew_grid(t2)), dim3(kThreads), 0, st, dcat, C2 / 4, (C2 + C1) / 4, t2, dx2);
    const int rc = io_check_launch("up2x_concat_bwd(split)");
    if (rc) return rc;
    hipLaunchKernelGGL(up2x_bwd_kernel, dim3(ew_grid(t1)), dim3(kThreads), 0, st, dcat, h, w, C2 / 4, C1 / 4, t1, dx1);
    return io_check_launch("up2x_concat_bwd");
}

extern "C" size_t io_unet_head_bwd_partial_floats(int P, int HW) {
    if (P <= 0 || HW <= 0) return 0;
    return (size_t)kHeadCols * (((size_t)P * HW + kThreads - 1) / kThreads);
}

extern "C" int io_unet_head_bwd(const float* act, const float* wo, const float* bo, const uint8_t* target, const float* eraser,
                                int P, int HW, int Cs, float inmask_weight, float scale, const float* gscale, float* dx,
                                float* dwo, float* dbo, float* loss_sums, float* partials, size_t partial_floats,
                                hipStream_t st) {
    IO_REQUIRE(act && wo && bo && target && eraser && dx && dwo && dbo && partials && P > 0 && HW > 0, IO_ERR_SHAPE,
               "unet_head_bwd: P=%d HW=%d; every operand but gscale and loss_sums is required", P, HW);
    IO_REQUIRE(Cs == kHeadCs, IO_ERR_SHAPE, "unet_head_bwd: Cs=%d, the kernel is written for a stored width of %d", Cs, kHeadCs);
    const size_t total = (size_t)P * HW, nblocks = (total + kThreads - 1) / kThreads;
    IO_REQUIRE(nblocks < (1u << 31), IO_ERR_SHAPE, "unet_head_bwd: too many blocks");
    IO_REQUIRE(partial_floats >= io_unet_head_bwd_partial_floats(P, HW), IO_ERR_WORKSPACE, "unet_head_bwd: partials %zu < %zu floats",
               partial_floats, io_unet_head_bwd_partial_floats(P, HW));
    IoProfScope prof(IO_PROF_UNET, 8.0 * total * Cs, 4.0 * total * (2.0 * Cs + 2), st);
    hipLaunchKernelGGL(unet_head_bwd_kernel, dim3((unsigned)nblocks), dim3(kThreads), 0, st, act, wo, bo, target, eraser, total,
                       inmask_weight, scale, gscale, dx, partials);
    const int rc = io_check_launch("unet_head_bwd");
    if (rc) return rc;
    hipLaunchKernelGGL(unet_head_bwd_reduce_kernel, dim3(kHeadCols), dim3(kThreads), 0, st, partials, (int)nblocks, dwo, dbo,
                       loss_sums);
    return io_check_launch("unet_head_bwd_reduce");
}
