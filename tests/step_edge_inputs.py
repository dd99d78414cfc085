"""Input builders and fp64 references of tests/test_gpu_step_edges.py (CPU tensors only), kept importable without a GPU so
that tests/test_step_edges_cpu.py can assert that they still discriminate: BatchNorm inputs whose ReLU mask no rounding
can flip, max-pool inputs full of exact ties, and the by-hand references that stand in where torch refuses the shape."""
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1
TDT = {0: torch.float32, 1: torch.bfloat16}
# the distance from zero every pre-activation bn(y) keeps, per storage type (fp32 / bf16); the |mean| = 1000 sigma variant
# keeps 2e-3: the fp32 mean of values near 300 is itself only good to 1.5e-5 = 5e-5 sigma
MASK_MARGIN = {0: 1e-4, 1: 3e-2}
SHIFTED_MARGIN = 2e-3

# ---- BatchNorm ---------------------------------------------------------------------------------------------------------
# (rows per group Mg, groups G, channels C, storage types, id).  bn_rows_per_block: want = 1024 / G, rpb = max(ceil(Mg / want),
# min(Mg, 64)), nb = ceil(Mg / rpb); col_map(CV): TX = min(CV, 256) column threads, TY = 256 / TX row lanes, nq = ceil(CV / 256)
BN_SHAPES = [
    (1, 1, 8, (0, 1), "mg1-one-row"),                          # var = 0, rstd = 1 / sqrt(eps); bf16 backward: CV = 1
    (2, 3, 8, (0, 1), "mg2-g3-three-groups"),
    (63, 1, 4, (0,), "mg63-c4-ty256-idle-lanes"),              # fp32 only: TX = 1, TY = 256, 63 rows
    (63, 1, 8, (0, 1), "mg63-c8-ty128-idle-lanes"),            # stats / fp32: TY = 128; bf16 backward: CV = 1, TY = 256
    (65, 2, 32, (0, 1), "mg65-g2-nb2-last-block-one-row"),     # rpb = 64: the second block is its own pivot row
    (100, 1, 1024, (0, 1), "mg100-c1024-ty1-ragged-36"),       # fp32: TY = 1; blocks of 64 + 36 rows
    (130, 1, 2048, (0, 1), "mg130-c2048-nq2-ragged"),          # fp32: two quads per thread; blocks of 64 + 64 + 2
    (8200, 8, 8, (0, 1), "mg8200-g8-rpb65-nb127"),             # want = 128, rpb = 65 > 64, nb = 127, a 10-row tail
    (70001, 1, 8, (0, 1), "mg70001-rpb69-nb1015"),             # a 35-row tail; 16 trips of bn_finalize, 2 of bn_bwd_finalize
]
SHIFTED = (100, 1, 1024)            # also run with mean = 1000 sigma (fp32)
APPLY_ONLY_SHAPES = [(3, 1, 2048, (0, 1), "mg3-c2048-apply-chunks-out-of-range")]      # per_group < 4 * grid stride
G9 = (65, 9, 32)                    # more groups than the cap bn_bwd_finalize_kernel once had


def rounded(t, dt):
    """fp64 copy of t after rounding to the storage type (the reference sees what the kernel sees)"""
    return t.float().to(TDT[dt]).double()


def bn_forward_ref(y, G, gamma, beta, rm0=None, rv0=None):
    """By hand (torch refuses one row per channel): y [G * Mg, C] fp64 -> dict of mean, var, rstd, scale, shift [G, C], the
    pre-activation [G * Mg, C] and the running estimates after the G groups in order.  Differentiable in y, gamma, beta.
    One row: var = 0 and the running variance moves towards it without the Mg / (Mg - 1) correction."""
    C = y.shape[1]
    yg = y.view(G, -1, C)
    Mg = yg.shape[1]
    mean = yg.mean(1)
    var = ((yg - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    pre = ((yg - mean[:, None]) * rstd[:, None] * gamma + beta).reshape(-1, C)
    out = dict(mean=mean, var=var, rstd=rstd, scale=rstd * gamma, shift=beta.expand(G, C), pre=pre)
    if rm0 is not None:
        rm, rv = rm0.clone(), rv0.clone()
        for g in range(G):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean[g].detach()
            rv = (1 - MOMENTUM) * rv + MOMENTUM * var[g].detach() * (Mg / (Mg - 1.0) if Mg > 1 else 1.0)
        out["rm"], out["rv"] = rm, rv
    return out


def bn_inputs(Mg, G, C, dt, shifted=False):
    """-> dict of fp64 CPU tensors, y / idt / yd / dout rounded to the storage type: y [G * Mg, C] such that no
    pre-activation bn(y) lies within the margin of zero (the offending elements are resampled until none is left), idt /
    yd (identity, input of the second BatchNorm), dout, gamma / beta with |beta| >= 0.1 (one row: bn(y) = beta), the
    initial running estimates, and the tables of the second BatchNorm [G, C]."""
    g = torch.Generator().manual_seed(1000 * Mg + 10 * C + G + dt + (7 if shifted else 0))
    M = G * Mg
    margin = SHIFTED_MARGIN if shifted else MASK_MARGIN[dt]
    off = 300.0 if shifted else 0.2

    def draw(n):
        return rounded(torch.randn(n, generator=g, dtype=torch.float64) * 0.3 + off, dt)
    gamma = (1 + 0.2 * (torch.rand(C, generator=g, dtype=torch.float64) - 0.5)).float().double()
    sign = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    beta = (sign * (0.1 + 0.15 * torch.rand(C, generator=g, dtype=torch.float64))).float().double()
    y = draw(M * C).view(M, C)
    for _ in range(200):
        bad = bn_forward_ref(y, G, gamma, beta)["pre"].abs() < 2 * margin       # (resampled at twice the margin asserted)
        n = int(bad.sum())
        if n == 0:
            break
        y[bad] = draw(n)
    else:
        raise AssertionError("bn_inputs: the resampling did not converge")
    d = dict(y=y, gamma=gamma, beta=beta, margin=margin)
    d["idt"] = rounded(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
    d["yd"] = rounded(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
    d["dout"] = rounded(torch.randn(M, C, generator=g, dtype=torch.float64), dt)
    d["rm0"] = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float().double()
    d["rv0"] = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).float().double()
    d["mean2"] = (torch.randn(G, C, generator=g, dtype=torch.float64) * 0.3).float().double()
    d["scale2"] = (torch.randn(G, C, generator=g, dtype=torch.float64) * 0.7 + 0.3).float().double()
    d["shift2"] = (torch.randn(G, C, generator=g, dtype=torch.float64) * 0.5).float().double()
    return d


def bn_backward_ref(d, G, masked):
    """fp64 autograd through bn_forward_ref (+ ReLU): -> dy, dgamma, dbeta, dz (the masked dout)"""
    y = d["y"].clone().requires_grad_(True)
    gamma, beta = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    pre = bn_forward_ref(y, G, gamma, beta)["pre"]
    dz = d["dout"] * (pre.detach() > 0) if masked else d["dout"]
    dy, dg, db = torch.autograd.grad(pre, [y, gamma, beta], dz)
    return dy, dg, db, dz


def bn_coefs_ref(y, dz, G, gamma):
    """The three-table form of bn_bwd_finalize_kernel's comment in fp64: dy = A * dz + B * y + Cc per (group, channel) with
    A = gamma * rstd, B = -A * rstd * mean(dz * xhat), Cc = -A * mean(dz) - B * mean.  -> A, B, Cc [G, C]"""
    C = y.shape[1]
    yg, dg = y.view(G, -1, C), dz.view(G, -1, C)
    mean = yg.mean(1)
    rstd = 1.0 / torch.sqrt(((yg - mean[:, None]) ** 2).mean(1) + EPS)
    xhat = (yg - mean[:, None]) * rstd[:, None]
    A = gamma * rstd
    B = -A * rstd * (dg * xhat).mean(1)
    return A, B, -A * dg.mean(1) - B * mean


# ---- max-pool 3 x 3, stride 2, padding 1 -----------------------------------------------------------------------------------
# dt, C, id: which kernel form io_maxpool_fwd_t / _bwd_t launch (vec = 4 fp32 / 8 bf16 channels per 16-byte chunk)
POOL_FORMS = [
    (0, 64, "fp32-c64-rows-shift"),            # C / vec = 16: the column split is a shift
    (0, 12, "fp32-c12-rows-divide"),           # C / vec = 3: cv_shift < 0
    (0, 24, "fp32-c24-rows-divide"),           # C / vec = 6
    (1, 64, "bf16-c64-rows-shift"),            # C / vec = 8
    (1, 24, "bf16-c24-rows-divide"),           # C / vec = 3
    (1, 4, "bf16-c4-element"),                 # C % 8 == 4: the element-indexed kernels
    (1, 12, "bf16-c12-element"),
]
POOL_HW = [(1, 1), (1, 7), (2, 2), (9, 13)]
POOL_WIDE = (5, 40)            # with C = 64: Wo * CV = 20 * 16 = 320 (fp32) > 256 threads, a ragged second trip of the j loop
POOL_N = 3


def pool_cases():
    """-> [(dt, C, H, W, id)]"""
    out = [(dt, C, H, W, "%s-h%dw%d" % (name, H, W)) for dt, C, name in POOL_FORMS for H, W in POOL_HW]
    out += [(dt, 64, POOL_WIDE[0], POOL_WIDE[1], "%s-c64-rows-h5w40-two-trips" % ("bf16" if dt else "fp32")) for dt in (0, 1)]
    return out


def tied_pool_input(N, C, H, W, relu, seed):
    """x [N,C,H,W] fp64 with the three values -0.5, 0, 0.5 (exact in bf16), after a ReLU the two values 0 and 0.5: most
    windows hold their maximum more than once"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 3, (N, C, H, W), generator=g).double() - 1.0) * 0.5
    return F.relu(x) if relu else x


def pool_windows(x):
    """x [N,C,H,W] -> the nine taps of every window [N,C,Ho,Wo,9] in (kh, kw) order, -inf where a tap is in the padding,
    and the flat input index h * W + w of every tap (-1 in the padding)"""
    N, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    pos = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    pp = F.pad(pos, (1, 1, 1, 1), value=-1.0)
    taps = xp.unfold(2, 3, 2).unfold(3, 3, 2)
    tpos = pp.unfold(2, 3, 2).unfold(3, 3, 2)
    Ho, Wo = taps.shape[2:4]
    return taps.reshape(N, C, Ho, Wo, 9), tpos.reshape(1, 1, Ho, Wo, 9).long()


def tied_window_fraction(x):
    taps, _ = pool_windows(x)
    mx = taps.max(-1, keepdim=True)[0]
    return float(((taps == mx).sum(-1) > 1).double().mean())


def maxpool_bwd_by_hand(x, dy, last=False):
    """Gradient of max_pool2d(x, 3, 2, 1) with every window's gradient sent to its first (or last) maximum in (kh, kw)
    order.  A window of nothing but -inf keeps its first in-bounds tap."""
    N, C, H, W = x.shape
    taps, tpos = pool_windows(x)
    mx = taps.max(-1, keepdim=True)[0]
    k = torch.arange(9, dtype=torch.float64)
    hit = ((taps == mx) & (tpos >= 0)).double()
    pick = (hit * ((k + 1) if last else (9 - k))).argmax(-1, keepdim=True)       # the weights make the arg-max unique
    tgt = tpos.expand(N, C, -1, -1, -1).gather(-1, pick).reshape(N, C, -1)
    dx = torch.zeros(N, C, H * W, dtype=torch.float64)
    dx.scatter_add_(2, tgt, dy.reshape(N, C, -1))
    return dx.view(N, C, H, W)


def pool_xf_tables(G, C, seed):
    """mean / scale / shift [G, C] of the transform in front of the pooling: multiples of 0.5 / powers of two of either sign
    / multiples of 0.25, so that relu((x - mean) * scale + shift) is exact in fp32 and bf16 on tied_pool_input"""
    g = torch.Generator().manual_seed(seed)
    mean = (torch.randint(-1, 2, (G, C), generator=g).double()) * 0.5
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (G, C), generator=g)]
    scale = scale * (torch.randint(0, 2, (G, C), generator=g).double() * 2 - 1)
    shift = torch.randint(-2, 3, (G, C), generator=g).double() * 0.25
    return mean, scale, shift


def pool_xf_apply(x, G, mean, scale, shift):
    """relu((x - mean[g]) * scale[g] + shift[g]) with g = n // (N / G); mean may be None"""
    N, C = x.shape[:2]
    grp = torch.arange(N) // (N // G)
    v = lambda t: t[grp].view(N, C, 1, 1)          # noqa: E731
    return F.relu((x - (v(mean) if mean is not None else 0.0)) * v(scale) + v(shift))


# ---- average pool + heads ----------------------------------------------------------------------------------------------------
# N, HW, C, K0, K1: avgpool_fc_kernel has 256 threads x 4 channels; fc_bwd_weight_kernel 32 channels x 8 slices of n per block
HEAD_SHAPES = [
    (1, 1, 4, 1, 0, "n1-hw1-c4-k1"),                        # one thread has work; N < 8: seven idle slices
    (3, 49, 20, 2, 3, "n3-hw49-c20-two-heads"),             # C % 32 = 20: the c < C guard
    (9, 4, 1024, 4, 0, "n9-c1024-second-slice-trip"),       # C = 256 threads x 4; N = 9: slice 0 sums n = 0 and 8
    (2, 144, 1028, 2, 3, "n2-hw144-c1028-one-past-the-block"),      # C / 4 = 257: thread 0 owns two chunks; C % 32 = 4
    (2, 4, 2048, 1000, 0, "k1000-the-midas-encoder-head"),
]


# ---- order loss -----------------------------------------------------------------------------------------------------------------
def order_loss_inputs(Kocc, Kdep, ndir, B, weighted, seed):
    """-> z [ndir * B, K] fp64, occ_t [ndir * B, 2], dep_t [ndir * B] int64, ov.  weighted: ov [B] int64 with the values 2
    and -1 among the rows (they belong to neither subset) and a label outside the head on two of those rows in every
    direction group; otherwise ov is None (plain mean) and every label is valid"""
    g = torch.Generator().manual_seed(seed)
    N = ndir * B
    z = (torch.randn(N, Kocc + Kdep, generator=g, dtype=torch.float64) * 2).float().double()
    occ_t = (torch.rand(N, 2, generator=g) < 0.4).double()
    dep_t = torch.randint(0, max(Kdep, 1), (N,), generator=g)
    ov = (torch.rand(B, generator=g) < 0.5).long()
    if not weighted:
        return z, occ_t, dep_t, None
    ov[3], ov[B - 1], ov[100] = 2, -1, 2
    for d in range(ndir):
        dep_t[d * B + 3] = Kdep + 5              # not looked at: the row carries no weight
        dep_t[d * B + B - 1] = -1
    return z, occ_t, dep_t, ov
