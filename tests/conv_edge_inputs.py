"""Case table, restated launcher predicates and fp64 references of tests/test_gpu_conv_edges.py (CPU tensors only), kept
importable without a GPU so that tests/test_conv_edges_cpu.py can assert that every case still reaches the arm its id
names: the geometry edges of the dense implicit-GEMM family (csrc/conv_igemm.hip with conv_p256.hip / conv_halo3.hip in
front of it for bf16) in its three passes -- forward, data gradient (one launch per lattice class of the stride), filter
gradient (split-K).

The predicates below restate host code of csrc/; each cites the function and the line it restates (lines as of the
change that added this file).  They exist so that a retuned threshold makes a CPU guard fail instead of letting a GPU
case silently test another arm."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

TDT = {0: torch.float32, 1: torch.bfloat16}

# (N, H, W, Cin, Cout, R, S, stride, pad), id, group.  Group A: shapes the networks / ops.conv2d reach -- must compute right.
# Group B: shapes only the C ABI accepts -- right, or refused with nothing written.  Group W: the Winograd forms at their
# smallest (3x3, stride 1, pad 1, 64 -> 64).
TABLE = [
    ((2, 15, 9, 64, 64, 3, 3, 2, 1), "odd-map-s2-3x3-unequal-classes", "A"),
    ((2, 8, 10, 64, 128, 3, 3, 2, 0), "s2-3x3-pad0-last-row-col-unread", "A"),
    ((3, 7, 9, 128, 64, 1, 1, 2, 0), "s2-1x1-odd-map-three-classes-without-tap", "A"),
    ((2, 6, 11, 64, 64, 3, 3, 1, 0), "s1-3x3-pad0-output-smaller", "A"),
    ((1, 5, 6, 64, 64, 1, 1, 1, 1), "1x1-pad1-zero-border-not-nopad", "A"),
    ((1, 5, 6, 64, 64, 3, 3, 1, 2), "3x3-pad2-output-larger", "A"),
    ((130, 1, 1, 64, 64, 3, 3, 1, 1), "1x1-maps-fastdiv-d1-two-row-tails", "A"),
    ((70, 2, 2, 64, 64, 3, 3, 2, 1), "2x2-to-1x1-s2-3x3", "A"),
    ((3, 9, 1, 64, 64, 3, 3, 1, 1), "one-column-map-wo1", "A"),
    ((50, 3, 3, 64, 128, 3, 3, 1, 1), "3x3-maps-tile-spans-15-samples-m450", "A"),
    ((1, 47, 45, 64, 2048, 1, 1, 1, 0), "fwd-128-wide-67-row-tail-wgrad-short-split", "A"),
    ((1, 47, 45, 2048, 64, 1, 1, 1, 0), "dgrad-128-wide-67-row-tail-wgrad-short-split", "A"),
    ((1, 183, 181, 64, 512, 3, 3, 2, 1), "128-wide-s2-3x3-odd-92x91-wgrad-27-splits", "A"),
    ((5, 13, 11, 128, 128, 3, 3, 1, 1), "wgrad-tr-128x128-wo11-not-w4", "A"),
    ((9, 10, 10, 128, 256, 3, 3, 1, 1), "wgrad-tr-128x128-wo10-not-w4-three-splits", "A"),
    ((3, 33, 32, 128, 128, 3, 3, 2, 1), "wgrad-tr-128x128-w4-s2-odd-ho17", "A"),
    ((2, 7, 32, 64, 128, 3, 3, 1, 1), "wo32-odd-ho7-wgrad-wino-row-or-w32", "A"),
    ((2, 9, 12, 64, 64, 1, 3, 1, 1), "abi-1x3", "B"),
    ((2, 9, 12, 64, 64, 3, 1, 1, 1), "abi-3x1", "B"),
    ((2, 11, 13, 64, 64, 5, 5, 2, 2), "abi-5x5-s2", "B"),
    ((1, 14, 14, 64, 64, 7, 7, 2, 3), "abi-7x7-s2", "B"),
    ((2, 8, 6, 64, 64, 2, 2, 2, 0), "abi-2x2-s2", "B"),
    ((2, 10, 11, 64, 64, 3, 3, 3, 1), "abi-3x3-s3", "B"),
    ((32, 2, 2, 64, 64, 3, 3, 1, 1), "wino-f23-2-wide", "W"),
    ((16, 4, 4, 64, 64, 3, 3, 1, 1), "wino-f43-halo-at-96-4x4", "W"),
    ((8, 4, 8, 64, 64, 3, 3, 1, 1), "wino-f43-halo-at-96-4x8", "W"),
    ((16, 2, 8, 64, 64, 3, 3, 1, 1), "wino-f43-no-halo-128", "W"),
    ((1, 8, 8, 64, 64, 3, 3, 1, 1), "wino-wgrad-f23-single-ktile", "W"),
    ((1, 4, 16, 64, 64, 3, 3, 1, 1), "wino-wgrad-f43-single-ktile", "W"),
]
CASES = [c for c, _, _ in TABLE]
IDS = {c: i for c, i, _ in TABLE}
GROUP = {c: g for c, _, g in TABLE}
WINO_FWD = [c for c, i, g in TABLE if g == "W" and "wgrad" not in i]
WINO_WGRAD = [c for c, i, g in TABLE if g == "W" and "wgrad" in i]
WGRAD_WINO_SWITCH = (2, 7, 32, 64, 128, 3, 3, 1, 1)      # filter gradient run with io_set_winograd on and off

# fused forms on the smallest maps: (case, BatchNorm groups G)
FUSED = [((128, 1, 1, 64, 64, 3, 3, 1, 1), 1), ((256, 1, 1, 64, 64, 3, 3, 1, 1), 2), ((32, 2, 2, 64, 64, 3, 3, 1, 1), 1)]

# io_conv2d_fwd_resid_dt with out_bits: (N, H, W, Cin, Cout, G, dtype, route of io_debug_last_nt_route with every eligible
# bf16 shape on conv_p256 -- io_set_bf16_p256(3)).  conv_p256 declines 128 !| Cout (io_launch_conv_p256: `g.Co % 128 != 0`).
RESID = [((4, 8, 8, 256, 64, 2), 0, 0), ((4, 8, 8, 256, 64, 2), 1, 0), ((4, 8, 8, 256, 128, 1), 1, 1)]


def cdiv(a, b):
    return (a + b - 1) // b


def out_hw(case):
    N, H, W, Ci, Co, R, S, s, p = case
    return (H + 2 * p - R) // s + 1, (W + 2 * p - S) // s + 1


# ---- csrc/capi.hip:63 io_geom_fwd / :83 io_geom_dgrad (Th / Tw: :96-97) / :106 io_run_dgrad ------------------------------
def geom_fwd(case):
    N, H, W, Ci, Co, R, S, s, p = case
    Ho, Wo = out_hw(case)
    return dict(N=N, Hi=H, Wi=W, Ci=Ci, Ho=Ho, Wo=Wo, Co=Co, outH=Ho, outW=Wo, os=1, ooh=0, oow=0, **{"is": s}, Th=R, Tw=S,
                dh0=-p, dhs=1, dw0=-p, dws=1, r0=0, rs=1, s0=0, ss=1, S=S, wT=R * S)


def geom_dgrad(case, ph, pw):
    N, H, W, Ci, Co, R, S, s, p = case
    Hy, Wy = out_hw(case)
    rf, sf = (ph + p) % s, (pw + p) % s
    return dict(N=N, Hi=Hy, Wi=Wy, Ci=Co, Ho=(H - ph + s - 1) // s, Wo=(W - pw + s - 1) // s, Co=Ci, outH=H, outW=W, os=s,
                ooh=ph, oow=pw, **{"is": 1}, Th=(R - rf + s - 1) // s if rf < R else 0,
                Tw=(S - sf + s - 1) // s if sf < S else 0, dh0=(ph + p - rf) // s, dhs=-1, dw0=(pw + p - sf) // s, dws=-1,
                r0=rf, rs=s, s0=sf, ss=s, S=S, wT=R * S)


def dgrad_classes(case):
    """the launches of io_run_dgrad (capi.hip:112-122): [(ph, pw, geom)] of the classes that hold pixels"""
    s = case[7]
    out = []
    for ph in range(s):
        for pw in range(s):
            g = geom_dgrad(case, ph, pw)
            if g["Ho"] > 0 and g["Wo"] > 0:
                out.append((ph, pw, g))
    return out


def rows(g):
    return g["N"] * g["Ho"] * g["Wo"]


# ---- csrc/conv_igemm.hip:2920 io_launch_conv_nt -----------------------------------------------------------------------------
NT_SMALL_TILES = 256         # `small_tiles` (conv_igemm.hip:3012): the largest count of 128-wide tiles that still runs 64 wide


def nt_tile_width(g):
    """`bn` of io_launch_conv_nt (conv_igemm.hip:3015-3016, dense): 128 wide where that leaves more than NT_SMALL_TILES tiles"""
    tiles128 = cdiv(rows(g), 128) * (g["Co"] // 128)
    return 128 if g["Co"] % 128 == 0 and tiles128 > NT_SMALL_TILES else 64


def nt_lin(g):
    """`lin` of io_launch_conv_nt (conv_igemm.hip:3024-3026): the addressing-free dense 1x1 GEMM on whole tiles"""
    return (g["Th"] * g["Tw"] == 1 and g["is"] == 1 and g["os"] == 1 and g["dh0"] == 0 and g["dw0"] == 0 and
            g["Hi"] == g["Ho"] and g["Wi"] == g["Wo"] and g["outH"] == g["Ho"] and g["outW"] == g["Wo"] and rows(g) % 128 == 0)


def nt_nopad(g):
    """`nopad` of conv_nt_kernel (conv_igemm.hip:285-286): a 1x1 stride-1 launch whose rows are valid for every k-tile or
    for none"""
    return (g["Th"] == 1 and g["Tw"] == 1 and g["dh0"] == 0 and g["dw0"] == 0 and g["is"] == 1 and g["Hi"] >= g["Ho"] and
            g["Wi"] >= g["Wo"])


def nt_last_tile_rows(g):
    return rows(g) - (cdiv(rows(g), 128) - 1) * 128


def fastdiv_d1(g):
    """io_fastdiv's `d <= 1` arm (io_common.h:97) for the two divisors of the row decode: (Ho * Wo == 1, Wo == 1)"""
    return g["Ho"] * g["Wo"] == 1, g["Wo"] == 1


def wino_fwd_form(g):
    """the Winograd branch of io_launch_conv_nt (conv_igemm.hip:3032-3036, `wino4` :3039, `halo` :3054-3055) for a plain
    fp32 3x3 stride-1 same-size launch with a scratch: 'direct', 'f23', 'f43' or 'f43-halo', and the HALO staging bound
    (<= 96) where it applies"""
    M = rows(g)
    if not (g["Th"] == 3 and g["Tw"] == 3 and g["is"] == 1 and g["os"] == 1 and g["Hi"] == g["Ho"] and g["Wi"] == g["Wo"] and
            g["Wo"] % 2 == 0 and M % 128 == 0 and g["Ci"] % 32 == 0):
        return "direct", None
    if not (g["Wo"] % 4 == 0 and M % 256 == 0 and g["Ci"] % 16 == 0):       # `wino4`
        return "f23", None
    hw = g["Ho"] * g["Wo"]
    if not (g["Wo"] <= 64 and 256 % g["Wo"] == 0):
        return "f43", None
    if hw % 256 == 0:
        return "f43-halo", None
    if 256 % hw != 0:
        return "f43", None
    bound = (256 // hw) * (g["Ho"] + 2) * (g["Wo"] // 4)
    return ("f43-halo" if bound <= 96 else "f43"), bound


def bf16_nt_route(g, mask=False):
    """shape part of io_launch_conv_halo3 (2; conv_halo3.hip:1022-1029) / io_launch_conv_p256 (1; conv_p256.hip:592-593)
    for a plain bf16 launch with every eligible shape
    routed to them (io_set_bf16_p256(3)); 0 = conv_nt_kernel"""
    dense = g["os"] == 1 and g["Ho"] == g["outH"] and g["Wo"] == g["outW"]
    same3 = (g["Th"] == 3 and g["Tw"] == 3 and g["S"] == 3 and g["is"] == 1 and dense and g["Hi"] == g["Ho"] and
             g["Wi"] == g["Wo"] and g["dh0"] == -g["dhs"] and g["dw0"] == -g["dws"])
    if (same3 and not mask and g["Co"] == 64 and g["Ci"] in (64, 128) and g["Wo"] in (32, 64) and
            (g["Ho"] * g["Wo"]) % 256 == 0):
        return 2
    if dense and rows(g) % 256 == 0 and g["Ci"] % 64 == 0 and g["Co"] % 128 == 0 and g["Th"] * g["Tw"] >= 1:
        return 1
    return 0


# ---- csrc/conv_igemm.hip:2836 plan_wgrad / :2871 wgrad_wino_shape_ok / :2878 plan_wgrad_wino / :3187 io_launch_conv_wgrad --------
def plan_wgrad(g, fp32=True):
    M = rows(g)
    bmo = 128 if g["Co"] % 128 == 0 else 64
    bnc = 128 if g["Ci"] % 128 == 0 else 64
    tiles = max((g["Co"] // bmo) * g["Th"] * g["Tw"] * (g["Ci"] // bnc), 1)
    tr = fp32 and bmo == 128 and bnc == 128
    nkt = cdiv(M, 32)
    want = ((2304 if tiles >= 128 else 768) if tr else 1024) // tiles
    maxs = max(nkt // 8, 1)
    splits = max(min(want, maxs), 1)
    kps = cdiv(nkt, splits)
    splits = cdiv(nkt, kps)
    return dict(bmo=bmo, bnc=bnc, tiles=tiles, nkt=nkt, splits=splits, kps=kps, last_split=nkt - (splits - 1) * kps,
                last_rows=M - (nkt - 1) * 32)


def wgrad_wino_shape_ok(g):
    return (g["Th"] == 3 and g["Tw"] == 3 and g["is"] == 1 and g["os"] == 1 and g["Hi"] == g["Ho"] and g["Wi"] == g["Wo"] and
            g["dh0"] == -1 and g["dw0"] == -1 and g["Wo"] % 8 == 0 and rows(g) % 64 == 0 and g["Ci"] % 64 == 0 and
            g["Co"] % 64 == 0)


def plan_wgrad_wino(g):
    tiles = (g["Co"] // 64) * 3 * (g["Ci"] // 64)
    nkt = rows(g) // 64
    splits = max(min(1024 // tiles, max(nkt // 8, 1)), 1)
    kps = cdiv(nkt, splits)
    return dict(tiles=tiles, nkt=nkt, splits=cdiv(nkt, kps), kps=kps)


def wgrad_form(g, dt, wino_on=True):
    """the instantiation io_launch_conv_wgrad picks (halo3 / stem aside; conv_igemm.hip: F(4,3) by 16 | Wo :3238, `w32` :3274,
    W4 :3306, `w8` :3333, `trk` :3354-3355): fp32 'wino-f23' | 'wino-f43' | 'tr-w4' | 'tr' |
    'rows-w32' | 'rows'; bf16 'dma-tr' | 'w8' | 'rows'"""
    p = plan_wgrad(g, dt == 0)
    if dt == 0:
        if wino_on and wgrad_wino_shape_ok(g):
            return "wino-f43" if g["Wo"] % 16 == 0 else "wino-f23"
        if p["bmo"] == 128 and p["bnc"] == 128:
            return "tr-w4" if g["Wo"] % 4 == 0 else "tr"
        lin1x1 = g["Th"] * g["Tw"] == 1 and g["is"] == 1 and g["dh0"] == 0 and g["dw0"] == 0 and g["Hi"] == g["Ho"] and \
            g["Wi"] == g["Wo"]
        return "rows-w32" if (not lin1x1 and g["Wo"] % 32 == 0) else "rows"
    trk = rows(g) % 64 == 0 and (g["Ho"] * g["Wo"]) % 64 == 0 and g["Wo"] % (512 // p["bnc"]) == 0
    return "dma-tr" if trk else ("w8" if g["Wo"] % 8 == 0 else "rows")


def bf16_wgrad_route(g):
    """io_wgrad_halo3_shape (conv_halo3.hip:1217-1222): 2 = conv_wgrad_halo3_kernel, 0 = the kernels of conv_igemm.hip"""
    ok = (g["Th"] == 3 and g["Tw"] == 3 and g["is"] == 1 and g["Hi"] == g["Ho"] and g["Wi"] == g["Wo"] and g["Ci"] == g["Co"] and
          g["Ci"] in (64, 128, 256) and g["Wo"] in (64, 32, 16) and (g["Ho"] * g["Wo"]) % 128 == 0 and g["dh0"] == -1 and
          g["dw0"] == -1)
    return 2 if ok else 0


# ---- positions that are exactly zero, from the geometry alone ------------------------------------------------------------
def _read(size, out, k, s, p):
    """[size] bool: input index i is read by some window, i = o * s - p + r with 0 <= o < out, 0 <= r < k"""
    hit = np.zeros(size, dtype=bool)
    for o in range(out):
        for r in range(k):
            i = o * s - p + r
            if 0 <= i < size:
                hit[i] = True
    return hit


def dx_zero_positions(case):
    """[H, W] bool: input pixels no window reads -- a row or column past the last window, or a lattice class of the stride
    that no filter tap reaches.  The data gradient there is exactly 0 (exactly `add` where accumulating)."""
    N, H, W, Ci, Co, R, S, s, p = case
    Ho, Wo = out_hw(case)
    rr, cc = _read(H, Ho, R, s, p), _read(W, Wo, S, s, p)
    return torch.from_numpy(~(rr[:, None] & cc[None, :]))


def tapless_class_positions(case):
    """[H, W] bool from io_geom_dgrad's tap counts: pixels of the classes with Th == 0 or Tw == 0"""
    N, H, W, Ci, Co, R, S, s, p = case
    z = torch.zeros(H, W, dtype=torch.bool)
    for ph, pw, g in dgrad_classes(case):
        if g["Th"] == 0 or g["Tw"] == 0:
            z[ph::s, pw::s] = True
    return z


def y_zero_positions(case):
    """[Ho, Wo] bool: output pixels whose every tap lies in the padding (the border of a 1x1 convolution with pad 1)"""
    N, H, W, Ci, Co, R, S, s, p = case
    Ho, Wo = out_hw(case)
    rr = np.array([any(0 <= o * s - p + r < H for r in range(R)) for o in range(Ho)])
    cc = np.array([any(0 <= o * s - p + r < W for r in range(S)) for o in range(Wo)])
    return torch.from_numpy(~(rr[:, None] & cc[None, :]))


def dgrad_by_lattice(case, dy, w):
    """io_run_dgrad's decomposition emulated with fp64 torch: for every class (ph, pw), dx[ph::s, pw::s][ho, wo] = sum over
    the class's taps (th, tw) of dy[ho + dh0 - th, wo + dw0 - tw] . w[:, :, r0 + s th, s0 + s tw] (zero outside dy).
    dy [N, Co, Hy, Wy], w [Co, Ci, R, S] -> dx [N, Ci, H, W]"""
    N, H, W, Ci, Co, R, S, s, p = case
    dx = torch.full((N, Ci, H, W), float("nan"), dtype=torch.float64)
    Hy, Wy = dy.shape[2:]
    for ph, pw, g in dgrad_classes(case):
        acc = torch.zeros(N, Ci, g["Ho"], g["Wo"], dtype=torch.float64)
        for th in range(g["Th"]):
            for tw in range(g["Tw"]):
                r, q = g["r0"] + g["rs"] * th, g["s0"] + g["ss"] * tw
                dh, dw = g["dh0"] + g["dhs"] * th, g["dw0"] + g["dws"] * tw
                ho = torch.arange(g["Ho"]) + dh
                wo = torch.arange(g["Wo"]) + dw
                okh, okw = (ho >= 0) & (ho < Hy), (wo >= 0) & (wo < Wy)
                sub = dy[:, :, ho.clamp(0, Hy - 1)][:, :, :, wo.clamp(0, Wy - 1)]
                sub = sub * (okh[:, None] & okw[None, :]).double()
                acc += torch.einsum("nohw,oc->nchw", sub, w[:, :, r, q])
        dx[:, :, ph::s, pw::s] = acc
    return dx


# ---- inputs and references ---------------------------------------------------------------------------------------------------
def rounded(t, dt):
    """fp64 copy of t after rounding to the storage type (the reference sees what the kernel sees)"""
    return t.float().to(TDT[dt]).double()


@functools.lru_cache(maxsize=None)
def reference(case, dt):
    """-> dict of fp64 NCHW CPU tensors on seeded inputs rounded to the storage type: x, w, dy, add, act (the activation
    whose sign is the ReLU mask), and F.conv2d / autograd results y, gx, gw.  Computed once per (case, dt) and shared:
    callers must not modify it."""
    N, H, W, Ci, Co, R, S, s, p = case
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Ci + Co + 7 * R + s + p + dt)
    x = rounded(torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64), dt).requires_grad_(True)
    w = rounded(torch.randn(Co, Ci, R, S, generator=g, dtype=torch.float64) / np.sqrt(Ci * R * S), dt).requires_grad_(True)
    y = F.conv2d(x, w, stride=s, padding=p)
    dy = rounded(torch.randn(y.shape, generator=g, dtype=torch.float64), dt)
    gx, gw = torch.autograd.grad(y, [x, w], dy)
    add = rounded(torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64), dt)
    act = rounded(torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64), dt)
    return dict(x=x.detach(), w=w.detach(), dy=dy, add=add, act=act, y=y.detach(), gx=gx, gw=gw)


def worst(got, ref):
    """NCHW tensors -> (relative error = max |got - ref| / max |ref|, (n, h, w, c) of the worst element); a NaN in `got`
    counts as infinitely wrong"""
    d = (got.double() - ref.double()).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    i = int(d.argmax())
    n, c, h, w_ = np.unravel_index(i, tuple(d.shape))
    return float(d.reshape(-1)[i] / ref.abs().max().clamp_min(1e-30)), (int(n), int(h), int(w_), int(c))
