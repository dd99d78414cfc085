// COCO polygon instance masks -> dense uint8 masks, on the device (DESIGN.md "Polygon masks").
//
// The rule is the published COCO mask API's (rleFrPoly, and merge as a union), see include/instaorder_hip.h.  It is a
// PARITY rule: every crossing of an edge with a pixel-centre column toggles everything from its position to the end of the
// column-major plane, so a pixel is set iff an odd number of crossings lie at or before it.  That needs no sort:
//   1. poly_toggle_kernel    one block per part, one wave per edge (strided), one lane per walk step: the lane evaluates
//                            the two walk points of its step and flips bit a = x * H + y of the part's plane with a 32-bit
//                            atomicXor.  XOR commutes, so the order in which toggles land does not matter, and crossings
//                            at one position cancel in pairs as the rule says.
//   2. poly_scan_kernel      one block per part: inclusive prefix parity along the plane.  Inside a word five shift-xor
//                            steps; the carry into a word is the parity of all earlier words -- a __ballot of the word
//                            parities and a popcount below the lane inside a wave64, four wave parities through LDS
//                            inside the block, a running bit across the passes (IO_POLY_SCAN_WORDS words per pass).
//   3. poly_gather_kernel    as rle_decode_kernel: a thread owns one aligned 4-byte word of the row-major output, reads
//                            bit x * H + y of each of its pixels from every part of the instance, ORs and stores.
// poly_offsets_kernel in front computes where each part's plane starts (an exclusive prefix sum over the parts).
//
// The only floating-point work is the minor coordinate of a walk point, trunc(b + s * t + 0.5) in double with the
// product and both sums rounded separately, as the C original compiled without contraction does: contraction is off for
// this file.  Everything else, the row of a crossing included, is integer arithmetic: (Ymin + 0.5) / 5 - 0.5 =
// (Ymin - 2) / 5 is an integer only where the double expression is exact, and at least 0.2 away from one otherwise.
//
// Safety does not depend on the vertex values: coordinates are clamped to +-IO_POLY_MAX_COORD on load (no int overflow in
// the walk), a toggle happens only at a position inside the plane, and every store address comes from the descriptors
// the host validated.
#include "io_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;                // four wave64
constexpr int kWaves = kThreads / 64;
constexpr int kWordsPerThread = 4;           // gather: 16 output pixels per thread and chunk
constexpr int kChunkWords = kThreads * kWordsPerThread;
static_assert(IO_POLY_SCAN_WORDS == kThreads, "the scan takes one plane word per thread and pass");

__host__ __device__ inline unsigned long long plane_words(int H, int W) {
    return ((unsigned long long)H * (unsigned long long)W + 31ull) >> 5;
}

// off[p] = sum of plane_words over the parts before p (one block)
__global__ __launch_bounds__(kThreads) void poly_offsets_kernel(const io_poly_part* __restrict__ parts,
                                                                const io_poly_mask* __restrict__ masks, int n_parts,
                                                                unsigned long long* __restrict__ off) {
    __shared__ unsigned long long s[kThreads];
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < n_parts; base += kThreads) {       // block-uniform trip count
        const int p = base + tid;
        unsigned long long w = 0;
        if (p < n_parts) {
            const io_poly_mask m = masks[parts[p].mask];
            w = plane_words(m.H, m.W);
        }
        s[tid] = w;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {
            const unsigned long long v = tid >= d ? s[tid - d] : 0ull;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        if (p < n_parts) off[p] = carry + s[tid] - w;
        carry += s[kThreads - 1];
        __syncthreads();
    }
}

__device__ __forceinline__ int clamp_coord(int v) {
    return v < -IO_POLY_MAX_COORD ? -IO_POLY_MAX_COORD : (v > IO_POLY_MAX_COORD ? IO_POLY_MAX_COORD : v);
}

// minor coordinate of walk point t: three separately rounded double operations, then C's (int)
__device__ __forceinline__ int walk_minor(int b, double s, int t) {
    const double prod = s * (double)t;
    const double sum = (double)b + prod;
    return (int)(sum + 0.5);
}

__global__ __launch_bounds__(kThreads) void poly_toggle_kernel(const int32_t* __restrict__ verts,
                                                               const io_poly_part* __restrict__ parts,
                                                               const io_poly_mask* __restrict__ masks,
                                                               const unsigned long long* __restrict__ off,
                                                               uint32_t* __restrict__ planes) {
    const io_poly_part part = parts[blockIdx.x];
    const io_poly_mask m = masks[part.mask];
    const int H = m.H, W = m.W;
    const long HW = (long)H * W;
    uint32_t* plane = planes + off[blockIdx.x];
    const int32_t* v = verts + 2 * part.vert_off;
    const int k = part.n_verts;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < k; j += kWaves) {
        const int j1 = j + 1 == k ? 0 : j + 1;                   // the ring closes on its first vertex
        int xs = clamp_coord(v[2 * j]), ys = clamp_coord(v[2 * j + 1]);
        int xe = clamp_coord(v[2 * j1]), ye = clamp_coord(v[2 * j1 + 1]);
        const int dx = xe > xs ? xe - xs : xs - xe, dy = ye > ys ? ye - ys : ys - ye;
        const bool flat = dx >= dy;
        // the direction the C original walks in decides only the ORDER of the walk points; a crossing is a property of
        // two neighbouring points, so the normalised direction serves
        if (flat ? xs > xe : ys > ye) {
            int t = xs; xs = xe; xe = t;
            t = ys; ys = ye; ye = t;
        }
        const int n = flat ? dx : dy;
        if (n == 0) continue;                                    // one point, no crossing
        const double s = flat ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
        for (int t = 1 + lane; t <= n; t += 64) {                // n <= 2^25: no overflow
            int c, vmin;
            if (flat) {
                c = xs + t;                                      // u(t - 1) = c - 1
                const int v0 = walk_minor(ys, s, t - 1), v1 = walk_minor(ys, s, t);
                vmin = v0 < v1 ? v0 : v1;
            } else {
                const int u0 = walk_minor(xs, s, t - 1), u1 = walk_minor(xs, s, t);
                if (u0 == u1) continue;
                c = u0 > u1 ? u0 : u1;
                vmin = ys + t - 1;
            }
            if (c < 3) continue;
            const int c3 = c - 3;
            if (c3 % 5 != 0) continue;                           // not on a pixel centre
            const int x = c3 / 5;
            if (x >= W) continue;
            const int r = vmin - 2;                              // y = clamp(ceil(r / 5), 0, H)
            int y = r / 5 + (r % 5 > 0 ? 1 : 0);
            y = y < 0 ? 0 : (y > H ? H : y);
            const long a = (long)x * H + y;
            if (a >= HW) continue;                               // the position past the last pixel sets nothing
            atomicXor(plane + (a >> 5), 1u << (a & 31));
        }
    }
}

__global__ __launch_bounds__(kThreads) void poly_scan_kernel(const io_poly_part* __restrict__ parts,
                                                             const io_poly_mask* __restrict__ masks,
                                                             const unsigned long long* __restrict__ off,
                                                             uint32_t* __restrict__ planes) {
    __shared__ unsigned s_par[kWaves];
    const io_poly_mask m = masks[parts[blockIdx.x].mask];
    const long nw = (long)plane_words(m.H, m.W);
    uint32_t* plane = planes + off[blockIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned running = 0;                                        // parity of all words of earlier passes
    for (long base = 0; base < nw; base += IO_POLY_SCAN_WORDS) { // block-uniform trip count
        const long i = base + threadIdx.x;
        uint32_t w = i < nw ? plane[i] : 0u;
        w ^= w << 1;
        w ^= w << 2;
        w ^= w << 4;
        w ^= w << 8;
        w ^= w << 16;                                            // bit b = parity of bits 0 .. b
        const unsigned long long odd = __ballot((int)(w >> 31)); // the words of this wave with odd parity
        const unsigned below = (unsigned)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
        if (lane == 0) s_par[wave] = (unsigned)__popcll(odd) & 1u;
        __syncthreads();
        unsigned carry = running ^ below, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            if (k < wave) carry ^= s_par[k];
            all ^= s_par[k];
        }
        running ^= all;
        if (carry) w = ~w;
        if (i < nw) plane[i] = w;
        __syncthreads();                                         // s_par is rewritten by the next pass
    }
}

__global__ __launch_bounds__(kThreads) void poly_gather_kernel(const io_poly_mask* __restrict__ masks,
                                                               const unsigned long long* __restrict__ off,
                                                               const uint32_t* __restrict__ planes,
                                                               uint8_t* __restrict__ out) {
    const io_poly_mask d = masks[blockIdx.y];
    const int H = d.H, W = d.W;
    const long HW = (long)H * W;
    uint8_t* dst = out + d.out_off;
    const int head = (int)((uintptr_t)dst & 3);
    const long nwords = (HW + head + 3) >> 2;                    // aligned words that cover dst[0 .. HW)
    const unsigned value = (unsigned)d.value & 0xffu;
#pragma unroll
    for (int j = 0; j < kWordsPerThread; ++j) {
        const long w = (long)blockIdx.x * kChunkWords + j * kThreads + threadIdx.x;
        if (w >= nwords) break;
        const long p0 = 4 * w - head;
        const int k0 = p0 < 0 ? (int)-p0 : 0;
        const unsigned first = (unsigned)(p0 + k0);
        int y = (int)(first / (unsigned)W);
        int x = (int)first - y * W;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < k0 || p0 + k >= HW) continue;
            const unsigned q = (unsigned)x * (unsigned)H + (unsigned)y;    // < H * W < 2^31
            unsigned bit = 0;
            for (int p = 0; p < d.n_parts; ++p) bit |= planes[off[d.first_part + p] + (q >> 5)] >> (q & 31);
            if (bit & 1u) word |= value << (8 * k);
            if (++x == W) { x = 0; ++y; }
        }
        if (p0 >= 0 && p0 + 4 <= HW) {
            *reinterpret_cast<uint32_t*>(dst + p0) = word;
        } else {                                                 // first / last word of a mask: bytes outside it are not ours
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k >= 0 && p0 + k < HW) dst[p0 + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

struct PolyPlan {
    size_t header_bytes, plane_bytes;
    long max_words;          // aligned output words of the largest mask (+ one for a ragged head)
    double pixels;
};

// the checks that need no buffer; *plan filled on success
int poly_check_tables(const io_poly_part* parts, int n_parts, const io_poly_mask* masks, int n_masks, size_t n_verts,
                      bool check_verts, PolyPlan* plan) {
    IO_REQUIRE(n_masks > 0 && masks, IO_ERR_SHAPE, "poly_fill: empty batch or null mask table (n_masks=%d)", n_masks);
    IO_REQUIRE(n_masks <= 65535, IO_ERR_SHAPE, "poly_fill: n_masks=%d out of range (at most 65535 masks per launch)",
               n_masks);
    IO_REQUIRE(n_parts >= 0 && (n_parts == 0 || parts), IO_ERR_SHAPE, "poly_fill: n_parts=%d or null part table", n_parts);
    long owned = 0;
    unsigned long long words = 0;
    plan->max_words = 0;
    plan->pixels = 0.0;
    for (int i = 0; i < n_masks; ++i) {
        const io_poly_mask& d = masks[i];
        IO_REQUIRE(d.H > 0 && d.W > 0 && (long)d.H * d.W < (1L << 31), IO_ERR_SHAPE,
                   "poly_fill: mask %d has size %d x %d (need H, W > 0 and H * W < 2^31)", i, d.H, d.W);
        IO_REQUIRE(d.value >= 0 && d.value <= 255, IO_ERR_SHAPE, "poly_fill: mask %d value=%d does not fit a byte", i,
                   d.value);
        IO_REQUIRE(d.n_parts >= 0 && d.first_part >= 0 && d.first_part <= n_parts && d.n_parts <= n_parts - d.first_part,
                   IO_ERR_SHAPE, "poly_fill: mask %d parts [%d, +%d) outside the part table of %d", i, d.first_part,
                   d.n_parts, n_parts);
        for (int p = d.first_part; p < d.first_part + d.n_parts; ++p)
            IO_REQUIRE(parts[p].mask == i, IO_ERR_SHAPE, "poly_fill: part %d names mask %d but mask %d owns it", p,
                       parts[p].mask, i);
        owned += d.n_parts;
        const size_t hw = (size_t)d.H * (size_t)d.W;
        words += plane_words(d.H, d.W) * (unsigned long long)d.n_parts;
        plan->pixels += (double)hw;
        const long ow = ((long)hw + 3 + 3) / 4;
        if (ow > plan->max_words) plan->max_words = ow;
    }
    // a part names one mask, so the ranges above cannot overlap; together they must cover the table
    IO_REQUIRE(owned == n_parts, IO_ERR_SHAPE, "poly_fill: the masks own %ld parts, the part table has %d", owned, n_parts);
    for (int p = 0; p < n_parts; ++p) {
        const io_poly_part& q = parts[p];
        IO_REQUIRE(q.mask >= 0 && q.mask < n_masks, IO_ERR_SHAPE, "poly_fill: part %d names mask %d of %d", p, q.mask,
                   n_masks);
        IO_REQUIRE(q.n_verts >= 1, IO_ERR_SHAPE, "poly_fill: part %d has n_verts=%d (at least one vertex)", p, q.n_verts);
        if (check_verts)
            IO_REQUIRE(q.vert_off >= 0 && (size_t)q.vert_off <= n_verts && (size_t)q.n_verts <= n_verts - (size_t)q.vert_off,
                       IO_ERR_SHAPE, "poly_fill: part %d vertices outside the vertex buffer", p);
    }
    IO_REQUIRE(words < (1ull << 40), IO_ERR_SHAPE, "poly_fill: %llu plane words (the workspace would exceed 4 TiB)", words);
    plan->header_bytes = ((size_t)n_parts * sizeof(unsigned long long) + 15) / 16 * 16;
    plan->plane_bytes = (size_t)words * 4;
    return IO_OK;
}

}  // namespace

extern "C" int io_poly_scan_words(void) { return IO_POLY_SCAN_WORDS; }

extern "C" size_t io_poly_fill_workspace_bytes(const io_poly_part* parts_host, int n_parts, const io_poly_mask* masks_host,
                                               int n_masks) {
    PolyPlan plan;
    if (poly_check_tables(parts_host, n_parts, masks_host, n_masks, 0, false, &plan) != IO_OK) return 0;
    const size_t b = plan.header_bytes + plan.plane_bytes;
    return b < 16 ? 16 : b;
}

extern "C" int io_poly_fill_u8(const int32_t* verts_dev, size_t n_verts, const io_poly_part* parts_dev,
                               const io_poly_part* parts_host, int n_parts, const io_poly_mask* masks_dev,
                               const io_poly_mask* masks_host, int n_masks, uint8_t* out, size_t out_bytes, void* workspace,
                               size_t workspace_bytes, hipStream_t st) {
    IO_REQUIRE(masks_dev && out && workspace, IO_ERR_SHAPE, "poly_fill: null pointer");
    IO_REQUIRE(n_parts <= 0 || (verts_dev && parts_dev), IO_ERR_SHAPE, "poly_fill: null vertex or part table");
    PolyPlan plan;
    const int rc = poly_check_tables(parts_host, n_parts, masks_host, n_masks, n_verts, true, &plan);
    if (rc != IO_OK) return rc;
    for (int i = 0; i < n_masks; ++i) {
        const io_poly_mask& d = masks_host[i];
        const size_t hw = (size_t)d.H * (size_t)d.W;
        IO_REQUIRE(d.out_off >= 0 && (size_t)d.out_off <= out_bytes && hw <= out_bytes - (size_t)d.out_off, IO_ERR_SHAPE,
                   "poly_fill: mask %d output outside the output buffer", i);
    }
    const size_t need = plan.header_bytes + plan.plane_bytes;
    IO_REQUIRE(((uintptr_t)workspace & 15) == 0, IO_ERR_SHAPE, "poly_fill: workspace must be 16-byte aligned");
    IO_REQUIRE(workspace_bytes >= need, IO_ERR_WORKSPACE, "poly_fill: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    unsigned long long* off = static_cast<unsigned long long*>(workspace);
    uint32_t* planes = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + plan.header_bytes);
    if (n_parts > 0 && plan.plane_bytes) {
        const hipError_t e = hipMemsetAsync(planes, 0, plan.plane_bytes, st);
        IO_REQUIRE(e == hipSuccess, IO_ERR_LAUNCH, "poly_fill: clearing the planes: %s", hipGetErrorString(e));
    }
    IoProfScope prof(IO_PROF_POLY, 0.0, 8.0 * (double)n_verts + 3.0 * (double)plan.plane_bytes + plan.pixels, st);
    if (n_parts > 0) {
        hipLaunchKernelGGL(poly_offsets_kernel, dim3(1), dim3(kThreads), 0, st, parts_dev, masks_dev, n_parts, off);
        hipLaunchKernelGGL(poly_toggle_kernel, dim3(n_parts), dim3(kThreads), 0, st, verts_dev, parts_dev, masks_dev, off,
                           planes);
        hipLaunchKernelGGL(poly_scan_kernel, dim3(n_parts), dim3(kThreads), 0, st, parts_dev, masks_dev, off, planes);
    }
    const int gx = io_cdiv(plan.max_words, kChunkWords);
    hipLaunchKernelGGL(poly_gather_kernel, dim3(gx, n_masks), dim3(kThreads), 0, st, masks_dev, off, planes, out);
    return io_check_launch("poly_fill");
}
