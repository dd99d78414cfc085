// Bounding boxes and pixel counts of uint8 instance masks on the device: the reference's utils.mask_to_bbox for masks that
// exist only there (readers.COCOAReader keeps COCOA's visible masks encoded up to the device, so the box of a region --
// which the reference takes from its pixels -- cannot be computed on the host).
//
// io_mask_bbox_u8      masks [n][H][W] -> out int32 [n][5] = x, y, w, h, count of the pixels that satisfy the predicate
//                      (m == 1 or m != 0); a mask without such a pixel gives 0, 0, 0, 0, 0.  Three launches whatever n is:
//                      an init kernel sets out[i] to the identity (INT_MAX, INT_MAX, -1, -1, 0); one block per (row band,
//                      mask) turns 64 pixels of a row into one ballot per wave -- its lowest and highest set bit are the
//                      row's column extent inside that chunk, its popcount the pixels -- reduces the extents of its rows in
//                      the block and adds them to out[i] with integer atomicMin / atomicMax / atomicAdd, so the result does
//                      not depend on the order of the blocks; a finishing kernel turns (xmin, ymin, xmax, ymax) into x, y, w,
//                      h in place.  Mask i starts at byte i * H * W, which may be odd: the pixels are read as bytes, 64
//                      consecutive ones per wave instruction.
#include "io_common.h"

#include <limits.h>

namespace {

constexpr int kBT = 256;            // threads per block
constexpr int kBWaves = kBT / 64;
constexpr int kBandRows = 32;       // rows per block: wave w takes rows w, w + kBWaves, ... of the band
constexpr int kChunks = 4;          // 64-pixel chunks of a row in flight per wave

__global__ __launch_bounds__(64) void bbox_init_kernel(int n, int* __restrict__ acc) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int* a = acc + (size_t)i * 5;
    a[0] = INT_MAX;
    a[1] = INT_MAX;
    a[2] = -1;
    a[3] = -1;
    a[4] = 0;
}

__global__ __launch_bounds__(kBT) void bbox_band_kernel(const uint8_t* __restrict__ m, int H, int W, int eq1,
                                                        int* __restrict__ acc) {
    __shared__ int sred[kBWaves][5];
    const int i = blockIdx.y;
    const int y0 = blockIdx.x * kBandRows;
    const int y1 = y0 + kBandRows < H ? y0 + kBandRows : H;
    const uint8_t* mi = m + (size_t)i * ((size_t)H * W);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the loop bounds depend on the wave only, so every ballot sees a whole wave; the extents are the same in every lane
    int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1, cnt = 0;
    for (int y = y0 + wave; y < y1; y += kBWaves) {
        const uint8_t* row = mi + (size_t)y * W;
        int rmin = INT_MAX, rmax = -1;
        for (int x0 = 0; x0 < W; x0 += 64 * kChunks) {
            unsigned v[kChunks];
#pragma unroll
            for (int c = 0; c < kChunks; ++c) {
                const int x = x0 + c * 64 + lane;
                v[c] = x < W ? (unsigned)row[x] : 0u;        // 0 satisfies neither predicate
            }
#pragma unroll
            for (int c = 0; c < kChunks; ++c) {
                const unsigned long long b = __ballot(eq1 ? v[c] == 1u : v[c] != 0u);
                if (b) {
                    const int base = x0 + c * 64;
                    const int lo = base + __builtin_ctzll(b), hi = base + 63 - __builtin_clzll(b);
                    rmin = lo < rmin ? lo : rmin;
                    rmax = hi > rmax ? hi : rmax;
                    cnt += __popcll(b);
                }
            }
        }
        if (rmax >= 0) {
            xmin = rmin < xmin ? rmin : xmin;
            xmax = rmax > xmax ? rmax : xmax;
            ymin = y < ymin ? y : ymin;
            ymax = y;                                         // rows ascend
        }
    }
    if (lane == 0) {
        sred[wave][0] = xmin;
        sred[wave][1] = ymin;
        sred[wave][2] = xmax;
        sred[wave][3] = ymax;
        sred[wave][4] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kBWaves; ++k) {
        xmin = sred[k][0] < xmin ? sred[k][0] : xmin;
        ymin = sred[k][1] < ymin ? sred[k][1] : ymin;
        xmax = sred[k][2] > xmax ? sred[k][2] : xmax;
        ymax = sred[k][3] > ymax ? sred[k][3] : ymax;
        cnt += sred[k][4];
    }
    if (cnt == 0) return;
    int* a = acc + (size_t)i * 5;
    atomicMin(a + 0, xmin);
    atomicMin(a + 1, ymin);
    atomicMax(a + 2, xmax);
    atomicMax(a + 3, ymax);
    atomicAdd(a + 4, cnt);
}

__global__ __launch_bounds__(64) void bbox_finish_kernel(int n, int* __restrict__ acc) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int* a = acc + (size_t)i * 5;
    const int xmin = a[0], ymin = a[1], xmax = a[2], ymax = a[3], cnt = a[4];
    if (cnt == 0) {
        a[0] = a[1] = a[2] = a[3] = 0;                        // mask_to_bbox: [0, 0, 0, 0] for an empty mask
        return;
    }
    a[2] = xmax + 1 - xmin;
    a[3] = ymax + 1 - ymin;
}

}  // namespace

extern "C" int io_mask_bbox_band_rows(void) { return kBandRows; }

extern "C" int io_mask_bbox_u8(const uint8_t* masks, int n, int H, int W, int predicate, int32_t* out, hipStream_t st) {
    IO_REQUIRE(n >= 0 && n <= IO_MASK_MAX_N && H > 0 && W > 0 && (long)H * W < (1L << 31), IO_ERR_SHAPE,
               "mask_bbox_u8: n=%d H=%d W=%d", n, H, W);
    IO_REQUIRE(predicate == IO_MASK_NONZERO || predicate == IO_MASK_EQ1, IO_ERR_SHAPE, "mask_bbox_u8: predicate=%d", predicate);
    if (n == 0) return IO_OK;
    IO_REQUIRE(masks && out, IO_ERR_SHAPE, "mask_bbox_u8: null pointer");
    hipLaunchKernelGGL(bbox_init_kernel, dim3(io_cdiv(n, 64)), dim3(64), 0, st, n, out);
    hipLaunchKernelGGL(bbox_band_kernel, dim3(io_cdiv(H, kBandRows), n), dim3(kBT), 0, st, masks, H, W,
                       predicate == IO_MASK_EQ1 ? 1 : 0, out);
    hipLaunchKernelGGL(bbox_finish_kernel, dim3(io_cdiv(n, 64)), dim3(64), 0, st, n, out);
    return io_check_launch("mask_bbox_u8");
}
