"""A teacher-forced fp64 oracle of the ResNet-50 INFERENCE forward, unit by unit (test-only, plain torch on the CPU; imports
no GPU code).  tests/test_gpu_eval_units.py holds the eval executor (run_forward_eval of csrc/net.hip, through
io_net_forward_eval_taps) to it; tests/test_eval_units_cpu.py shows that the case table reaches what it names and that
the bars catch a wrong unit in its own unit.

The eval forward folds every BatchNorm into its convolution (fold_bn_kernel) and applies bias (+ identity) (+ ReLU) in the
convolution's epilogue.  It produces 54 tensors -- relu(conv1 + b), the max-pool output and per Bottleneck a1, a2, yd (where
the block has a downsample branch) and out -- and the logits: the 55 UNITS below, in execution order.  `reference`
recomputes each unit in float64 FROM THE STORED INPUT of that unit (the tap of the unit before it, converted exactly) and
the raw, unfolded parameters: relu(gamma * (conv(x, w) - mean) / sqrt(var + eps) + beta (+ identity)); so an error stays
in the unit that made it.

`make_state` gives the running estimates values at which the fold matters (the repository's seeded states have 0 / 1):
the batch mean / variance of one fp64 training-mode pass over the case's input (activations stay in range through all 53
layers), every variance times a seeded factor in [0.5, 2], every mean shifted by a seeded fraction (+-0.5) of its
standard deviation, and per BatchNorm three channels forced to the edges: running variance 1e-7 (eps decides the scale:
dropping it changes the channel tenfold; gamma of that channel is rescaled so that its output keeps its size), gamma < 0,
gamma = 0.

`emulate` is the oracle's own model of the dtype: fold in fp32, round the folded filter to the storage type, exact
products, fp32 bias, round the output to the storage type.  It exists only to measure the noise floor `ec` of the
comparison (emulation against the exact run on the emulation's own stored tensors; the code under test plays no part) and
to carry the seeded faults of tests/test_eval_units_cpu.py.  Bar of a unit: step_block_oracle.bar(ec, floor) = 3 ec + floor,
floors 6e-3 (bf16 tensor) / 2e-5 (fp32 tensor) / 1e-5 (logits).

`predict` lists the 53 convolution launches of a case and the kernel family each goes to, from the launcher predicates
restated in tests/conv_edge_inputs.py plus io_stem_rows_ok (csrc/stem.hip), the stem_halo predicate and the fill rule of
the persistent bf16 kernels (csrc/conv_halo3.hip, csrc/conv_p256.hip)."""
import functools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import conv_edge_inputs as cei
import step_block_oracle as sbo
from helpers import synthetic

BN_EPS = 1e-5
HEADS = [2, 3]
SEED = 523
PLANES = (64, 128, 256, 512)
NCU = 256                      # the launch predictions below hold on 256 CUs (the fill rule of the persistent kernels)

# (dtype, N, H, W, io_set_bf16_p256 modes (bf16; the first is the one a plain run of the case takes), units the oracle
# covers (None: all 55; an int: the first that many -- stem, pool and layer 1 at the one case whose point is a launch
# of layer 1 and whose full fp64 recomputation would take a minute))
CASES = [
    ("fp32", 2, 64, 64, (), None),
    ("fp32", 1, 32, 256, (), None),
    ("fp32", 4, 96, 64, (), None),
    ("fp32", 8, 32, 64, (), None),
    ("fp32", 17, 128, 128, (), 12),
    ("bf16", 2, 32, 256, (3, 0), None),
    ("bf16", 2, 64, 128, (3, 0), None),
    ("bf16", 3, 64, 64, (3, 1), None),
]


def case_id(case):
    return "%s-n%d-%dx%d" % case[:4]


# ---- the units ---------------------------------------------------------------------------------------------------------
def _units():
    U = [dict(name="stem", kind="conv", conv="conv1", bn="bn1", src=-1, idt=None, relu=True, stride=2, pad=3, k=7, cin=5,
              cout=64, block=None),
         dict(name="pool", kind="pool", src=0, cout=64, block=None)]
    x, inC = 1, 64
    for li, bi in sbo.BLOCKS:
        p = "layer%d.%d" % (li + 1, bi)
        stride, pl = (2 if (bi == 0 and li > 0) else 1), PLANES[li]
        a1 = len(U)
        U.append(dict(name=p + ".a1", kind="conv", conv=p + ".conv1", bn=p + ".bn1", src=x, idt=None, relu=True, stride=1,
                      pad=0, k=1, cin=inC, cout=pl, block=p))
        U.append(dict(name=p + ".a2", kind="conv", conv=p + ".conv2", bn=p + ".bn2", src=a1, idt=None, relu=True,
                      stride=stride, pad=1, k=3, cin=pl, cout=pl, block=p))
        idt = x
        if bi == 0:
            idt = len(U)
            U.append(dict(name=p + ".yd", kind="conv", conv=p + ".downsample.0", bn=p + ".downsample.1", src=x, idt=None,
                          relu=False, stride=stride, pad=0, k=1, cin=inC, cout=4 * pl, block=p))
        U.append(dict(name=p + ".out", kind="conv", conv=p + ".conv3", bn=p + ".bn3", src=a1 + 1, idt=idt, relu=True,
                      stride=1, pad=0, k=1, cin=pl, cout=4 * pl, block=p, block_in=x))
        x, inC = len(U) - 1, 4 * pl
    U.append(dict(name="logits", kind="head", src=x, block=None))
    return U


UNITS = _units()
NUNITS = len(UNITS)                              # 55: 54 tensors + logits
NTAPS = NUNITS - 1
UNIT_NAMES = [u["name"] for u in UNITS]
CONV_UNITS = [i for i, u in enumerate(UNITS) if u["kind"] == "conv"]        # the 53 conv_folded launches, in order
BN_NAMES = [UNITS[i]["bn"] for i in CONV_UNITS]
assert NUNITS == 55 and len(CONV_UNITS) == 53


def unit_shapes(N, H, W):
    """[(C, h, w)] of the 54 tensors"""
    out = []
    for u in UNITS[:-1]:
        if u["kind"] == "pool":
            out.append((64, H // 4, W // 4))
            continue
        c, h, w = (None, H, W) if u["src"] < 0 else out[u["src"]]
        out.append((u["cout"], (h + 2 * u["pad"] - u["k"]) // u["stride"] + 1, (w + 2 * u["pad"] - u["k"]) // u["stride"] + 1))
    return out


def geometries(N, H, W):
    """the conv_edge_inputs case tuple (N, H, W, Cin, Cout, R, S, stride, pad) of each of the 53 launches
    (run_forward_eval: io_geom_fwd(N, H, W, cin_store, ...); the stem reads the packed 8-channel input)"""
    shp = unit_shapes(N, H, W)
    out = []
    for i in CONV_UNITS:
        u = UNITS[i]
        c, h, w = (8, H, W) if u["src"] < 0 else shp[u["src"]]
        out.append((N, h, w, c, u["cout"], u["k"], u["k"], u["stride"], u["pad"]))
    return out


def floor_of(dtype, unit):
    if unit == NUNITS - 1:
        return sbo.FLOOR_LOGITS
    return sbo.FLOOR_BF16 if dtype == "bf16" else sbo.FLOOR_F32


# ---- inputs and state --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_state():
    """kaiming weights (synthetic.make_state_dict), as tests/test_gpu_step_blocks.py uses"""
    sd = synthetic.make_state_dict(SEED, 5, HEADS, style="kaiming")
    return sd, sbo.state64(sd)


@functools.lru_cache(maxsize=None)
def make_input(dtype, N, H, W):
    """x5[N, 5, H, W] float32 (modal1, modal2, rgb: a seeded pair batch at the larger side, cropped) and the same values
    as the net reads them (rounded to the storage type), float64"""
    S = max(H, W)
    b = synthetic.make_pair_batch(SEED + 7 * N + H + 3 * W, N, S)
    x5 = torch.from_numpy(np.concatenate([b["modal1"], b["modal2"], b["rgb"]], 1))[:, :, :H, :W].contiguous()
    return x5, sbo.round_fn(dtype)(x5.double())


def _f32(t):
    return t.float().double()


def _train_stats(state, x):
    """one fp64 training-mode pass: BatchNorm name -> (batch mean, biased batch variance)"""
    stats = OrderedDict()
    acts = []
    for u in UNITS[:-1]:
        if u["kind"] == "pool":
            acts.append(F.max_pool2d(acts[u["src"]], 3, 2, 1))
            continue
        xin = x if u["src"] < 0 else acts[u["src"]]
        y = F.conv2d(xin, state[u["conv"] + ".weight"], stride=u["stride"], padding=u["pad"])
        mean = y.mean(dim=(0, 2, 3))
        var = y.var(dim=(0, 2, 3), unbiased=False)
        stats[u["bn"]] = (mean, var)
        C = y.shape[1]
        z = (y - mean.view(1, C, 1, 1)) / torch.sqrt(var.view(1, C, 1, 1) + BN_EPS)
        z = z * state[u["bn"] + ".weight"].view(1, C, 1, 1) + state[u["bn"] + ".bias"].view(1, C, 1, 1)
        if u["idt"] is not None:
            z = z + acts[u["idt"]]
        acts.append(F.relu(z) if u["relu"] else z)
    return stats


EDGE_VAR = 1e-7
STAT_SAMPLES = 8               # the statistics pass reads at most this many samples of the case's input (all, but at N = 17)


def edge_channels(bn_index, C):
    """the three forced channels of BatchNorm `bn_index` (order of BN_NAMES): (variance 1e-7, gamma < 0, gamma = 0)"""
    r = np.random.RandomState(SEED + 31 * bn_index)
    c = r.choice(C, 3, replace=False)
    return int(c[0]), int(c[1]), int(c[2])


@functools.lru_cache(maxsize=None)
def make_state(dtype, N, H, W):
    """-> OrderedDict name -> float64 tensor of fp32-representable values (see the module docstring).  The statistics
    pass reads the first STAT_SAMPLES samples: the estimates only have to put the activations in range."""
    state = OrderedDict((k, v.clone()) for k, v in base_state()[1].items())
    for j, bn in enumerate(BN_NAMES):
        C = state[bn + ".weight"].numel()
        _, c_neg, c_zero = edge_channels(j, C)
        g = state[bn + ".weight"]
        g[c_neg] = -g[c_neg].abs().clamp_min(0.25)
        g[c_zero] = 0.0
    x = make_input(dtype, N, H, W)[1]
    stats = _train_stats(state, x[:STAT_SAMPLES])
    gen = torch.Generator().manual_seed(SEED + N + H + W)
    for j, bn in enumerate(BN_NAMES):
        mean, var = stats[bn]
        C = mean.numel()
        fac = 0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64)
        frac = torch.rand(C, generator=gen, dtype=torch.float64) - 0.5
        rm = mean + frac * torch.sqrt(var)
        rv = var * fac
        c_eps = edge_channels(j, C)[0]
        g = state[bn + ".weight"]
        # variance 1e-7: eps decides the scale; gamma rescaled so that gamma / sqrt(var + eps) stays what it was
        g[c_eps] = g[c_eps] * torch.sqrt((EDGE_VAR + BN_EPS) / (rv[c_eps] + BN_EPS))
        rv[c_eps] = EDGE_VAR
        state[bn + ".weight"] = _f32(g)
        state[bn + ".running_mean"] = _f32(rm)
        state[bn + ".running_var"] = _f32(rv)
    return state


def state_dict_of(state):
    """-> name -> float32 tensor, with the counters load_state_dict(strict=True) wants"""
    sd = base_state()[0]
    return OrderedDict((k, torch.from_numpy(np.array(v, copy=True)) if k.endswith("num_batches_tracked")
                        else state[k].float().reshape(v.shape)) for k, v in sd.items())


# ---- one unit, exact and emulated ----------------------------------------------------------------------------------------
def _head(state, x):
    feat = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    return torch.cat([F.linear(feat, state["fc_occ.weight"], state["fc_occ.bias"]),
                      F.linear(feat, state["fc_depth.weight"], state["fc_depth.bias"])], 1)


def exact_unit(state, i, xin, idt):
    """unit i in float64 from its input (and identity): the raw, unfolded parameters"""
    u = UNITS[i]
    if u["kind"] == "pool":
        return F.max_pool2d(xin, 3, 2, 1)
    if u["kind"] == "head":
        return _head(state, xin)
    y = F.conv2d(xin, state[u["conv"] + ".weight"], stride=u["stride"], padding=u["pad"])
    C = y.shape[1]
    v = lambda k: state[u["bn"] + k].view(1, C, 1, 1)      # noqa: E731
    z = v(".weight") * (y - v(".running_mean")) / torch.sqrt(v(".running_var") + BN_EPS) + v(".bias")
    if idt is not None:
        z = z + idt
    return F.relu(z) if u["relu"] else z


FAULTS = ("no_eps", "no_mean", "bias_shift64", "no_relu", "wrong_identity", "missing_tap_row", "swap_hw")


def _as_buffer(t, shape):
    """the NHWC memory of NCHW tensor t read as an NHWC tensor of NCHW `shape` (repeated where it is shorter)"""
    flat = t.permute(0, 2, 3, 1).reshape(-1)
    n = int(np.prod(shape))
    flat = flat.repeat((n + flat.numel() - 1) // flat.numel())[:n]
    N, C, H, W = shape
    return flat.reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous()


def emu_unit(state, i, xin, idt, rnd, fault=None, block_in=None):
    """unit i as the eval executor computes it in the dtype of `rnd`: scale and bias folded in fp32, the folded filter
    rounded to the storage type, exact products, fp32 bias, the output rounded to the storage type.  fault: one of FAULTS"""
    u = UNITS[i]
    if u["kind"] == "pool":
        return rnd(F.max_pool2d(xin, 3, 2, 1))
    if u["kind"] == "head":
        return _head(state, xin)
    f = lambda k: state[u["bn"] + k].float()               # noqa: E731
    eps = torch.tensor(0.0 if fault == "no_eps" else BN_EPS, dtype=torch.float32)
    s = f(".weight") / torch.sqrt(f(".running_var") + eps)
    bias = f(".bias") if fault == "no_mean" else f(".bias") - f(".running_mean") * s
    if fault == "bias_shift64":
        bias = torch.roll(bias, 64)
    w = rnd((state[u["conv"] + ".weight"].float() * s.view(-1, 1, 1, 1)).double())
    if fault == "swap_hw":                                 # the launch built with the two sides of the map exchanged
        N, C, H, W = xin.shape
        xin = xin.permute(0, 2, 3, 1).reshape(N, W, H, C).permute(0, 3, 1, 2)
    y = F.conv2d(xin, w, stride=u["stride"], padding=u["pad"])
    if fault == "missing_tap_row":                         # the input's last row never reaches the filter's bottom row
        xl = torch.zeros_like(xin)
        xl[:, :, -1] = xin[:, :, -1]
        wl = torch.zeros_like(w)
        wl[:, :, -1] = w[:, :, -1]
        y = y - F.conv2d(xl, wl, stride=u["stride"], padding=u["pad"])
    if fault == "swap_hw":
        N, C, H, W = y.shape
        y = y.permute(0, 2, 3, 1).reshape(N, W, H, C).permute(0, 3, 1, 2)
    z = y + bias.double().view(1, -1, 1, 1)
    if idt is not None:
        z = z + (_as_buffer(block_in, tuple(z.shape)) if fault == "wrong_identity" else idt)
    return rnd(z if (not u["relu"] or fault == "no_relu") else F.relu(z))


def _src(stored, x, i):
    u = UNITS[i]
    xin = x if u["src"] < 0 else stored[u["src"]]
    idt = stored[u["idt"]] if u.get("idt") is not None else None
    return xin, idt


def reference(state, x, stored, upto=None):
    """stored: the 54 tensors of a run (NCHW float64; entries past `upto` may be None) -> the first `upto` (default all
    55) units recomputed in float64, each from ITS stored input"""
    n = NUNITS if upto is None else upto
    return [exact_unit(state, i, *_src(stored, x, i)) for i in range(n)]


def emulate(state, x, dtype, upto=None):
    """a free-running emulated forward -> the first `upto` units as it would store them (logits exact from the last
    stored block)"""
    rnd = sbo.round_fn(dtype)
    n = NUNITS if upto is None else upto
    acts = []
    for i in range(n):
        acts.append(emu_unit(state, i, *_src(acts, x, i), rnd))
    return acts


def errors(got, ref):
    return [sbo.err_max(g, r) for g, r in zip(got, ref)]


@functools.lru_cache(maxsize=None)
def noise_floor(dtype, N, H, W, upto=None):
    """ec of the first `upto` units: the emulation held to the exact recomputation on the emulation's own stored tensors.
    -> (ec list, the emulation's stored tensors)"""
    state, x = make_state(dtype, N, H, W), make_input(dtype, N, H, W)[1]
    acts = emulate(state, x, dtype, upto)
    return errors(acts, reference(state, x, acts, len(acts))), acts


def bars(dtype, ec):
    return [sbo.bar(e, floor_of(dtype, i)) for i, e in enumerate(ec)]


def consumers(i):
    return [j for j, u in enumerate(UNITS) if u.get("src") == i or u.get("idt") == i]


def faulted_errors(dtype, N, H, W, fault, i):
    """The emulated run with `fault` built into unit i: errors of unit i and of every unit that reads it (each against
    the exact recomputation from the faulty run's own stored tensors).  Every other unit of that run reads what the clean
    emulation stored and computes what it computed.  -> {unit: error}"""
    state, x = make_state(dtype, N, H, W), make_input(dtype, N, H, W)[1]
    rnd = sbo.round_fn(dtype)
    acts = list(noise_floor(dtype, N, H, W)[1])
    u = UNITS[i]
    xin, idt = _src(acts, x, i)
    acts[i] = emu_unit(state, i, xin, idt, rnd, fault, acts[u["block_in"]] if "block_in" in u else None)
    out = {i: sbo.err_max(acts[i], exact_unit(state, i, xin, idt))}
    for j in consumers(i):
        xin, idt = _src(acts, x, j)
        out[j] = sbo.err_max(emu_unit(state, j, xin, idt, rnd), exact_unit(state, j, xin, idt))
    return out


# ---- launch predictions ----------------------------------------------------------------------------------------------------
def stem_rows_ok(g):
    """io_stem_rows_ok (csrc/stem.hip:399) for the exact-K fp32 stem launch run_forward_eval builds (cr = 5)"""
    return (g["Ci"] == 8 and g["Co"] == 64 and g["Th"] == 7 and g["Tw"] == 7 and g["is"] == 2 and g["os"] == 1 and
            g["dh0"] == -3 and g["dw0"] == -3 and g["Wo"] % 128 == 0 and 2 * g["Ho"] == g["Hi"] and 2 * g["Wo"] == g["Wi"])


def persist_fill_ok(tiles, mode, ncu=NCU):
    """the fill rule of the persistent bf16 kernels (p256_rounds_ok, csrc/conv_p256.hip:540; the same rule in
    io_launch_conv_halo3 / io_launch_conv_stem_halo): mode 3 takes every eligible launch, mode 1 only where at least
    80 % of the rounds' slots are used"""
    rounds = cei.cdiv(tiles, ncu)
    return mode == 3 or tiles * 10 >= rounds * ncu * 8


def stem_halo_shape(g):
    """shape part of io_launch_conv_stem_halo (csrc/conv_halo3.hip:1101-1103)"""
    return (g["Th"] == 7 and g["Tw"] == 7 and g["is"] == 2 and g["os"] == 1 and g["Ci"] == 8 and g["Co"] == 64 and
            g["Wo"] == 128 and g["Wi"] == 256 and g["Hi"] == 2 * g["Ho"] and g["Ho"] % 2 == 0 and g["dh0"] == -3 and
            g["dw0"] == -3)


def predict(dtype, N, H, W, mode=1, wino=True, ncu=NCU):
    """-> 53 dicts(unit, route = what io_debug_last_nt_route reports, family, tags): the launch io_launch_conv_nt makes
    of each conv_folded call.  tags name the arms the case table is there for (COVERAGE)."""
    out = []
    for i, case in zip(CONV_UNITS, geometries(N, H, W)):
        u, g = UNITS[i], cei.geom_fwd(case)
        M, tags, route = cei.rows(g), set(), 0
        add = u["idt"] is not None
        if dtype == "fp32":
            if u["k"] == 7:
                fam = "stem-rows" if stem_rows_ok(g) else "stem-exact"
                tags.add(fam)
                if fam == "stem-rows" and g["Ho"] != g["Wo"]:
                    tags.add("stem-rows-rect")
            elif u["k"] == 3:
                form, bound = cei.wino_fwd_form(g) if (wino and u["stride"] == 1) else ("direct", None)
                fam = "wino-" + form if form != "direct" else "nt64-3x3" + ("-s2" if u["stride"] == 2 else "")
                if form == "f43-halo":
                    tags.add("f43-halo")
                    if bound is not None:
                        tags.add("f43-halo-several-samples-per-tile")
                    if bound == 96:
                        tags.add("f43-halo-at-bound-96")
                    if g["Ho"] != g["Wo"]:
                        tags.add("f43-halo-rect")
                elif form == "f43":
                    tags.add("f43-no-halo")
                elif form == "f23":
                    tags.add("f23")
                    if g["Ho"] != g["Wo"]:
                        tags.add("f23-rect")
                elif u["stride"] == 1 and M % 128 != 0:
                    tags.add("direct-3x3-ragged-rows")
                if u["stride"] == 1 and g["Ho"] == 1:
                    tags.add("3x3-one-row-map")
                if u["stride"] == 1 and (g["Ho"], g["Wo"]) == (3, 2):
                    tags.add("3x3-odd-map-3x2")
            else:
                bn = cei.nt_tile_width(g)
                fam = "nt%d-1x1%s" % (bn, "-lin" if cei.nt_lin(g) else "")
                if cei.nt_last_tile_rows(g) in (32, 8):
                    tags.add("1x1-ragged-tile-%d-rows" % cei.nt_last_tile_rows(g))
                if bn == 128 and add and u["relu"]:
                    tags.add("nt128-bias-add-relu")
        else:
            persist = mode in (1, 3)
            r3 = cei.bf16_nt_route(g) if u["k"] != 7 else 0
            if u["k"] == 7:
                take = persist and stem_halo_shape(g) and persist_fill_ok(M // 256, mode, ncu)
                fam, route = ("stem-halo", 3) if take else ("stem-nt", 0)
                tags.add("stem-halo-rect" if (take and g["Ho"] != g["Wo"]) else fam)
                if stem_halo_shape(g) and mode == 1 and not take:
                    tags.add("mode1-fill-rule-declines")
            elif r3 == 2 and persist and persist_fill_ok(M // 256, mode, ncu):
                fam, route = "halo3-w%d%s" % (g["Wo"], "-breg" if g["Ci"] == 64 else ""), 2
                tags.add(fam)
            elif r3 in (1, 2) and mode != 0 and g["Co"] % 128 == 0 and persist_fill_ok(
                    (M // 256) * (g["Co"] // (256 if g["Co"] % 256 == 0 else 128)), mode, ncu):
                fam, route = "p256", 1
                tags.add("p256-bias-add" if add else "p256-bias")
                if (M // 256) % 2 == 1 and M // 256 > 1:
                    tags.add("p256-odd-tile-count")
            else:
                fam = "nt%d-%dx%d" % (cei.nt_tile_width(g), u["k"], u["k"])
                if r3 and mode == 1:
                    tags.add("mode1-fill-rule-declines")
        out.append(dict(unit=i, route=route, family=fam, tags=tags))
    return out


# what the case table is there for: every name must be predicted for at least one launch of one case
COVERAGE = ["stem-exact", "stem-rows-rect", "f43-halo", "f43-halo-rect", "f43-halo-several-samples-per-tile",
            "f43-halo-at-bound-96", "f43-no-halo", "f23", "f23-rect", "direct-3x3-ragged-rows", "3x3-one-row-map",
            "3x3-odd-map-3x2", "1x1-ragged-tile-32-rows", "1x1-ragged-tile-8-rows", "nt128-bias-add-relu",
            "stem-halo-rect", "stem-nt", "halo3-w64-breg", "halo3-w32-breg", "p256-bias", "p256-bias-add",
            "p256-odd-tile-count", "mode1-fill-rule-declines"]


def wino_units(dtype, N, H, W):
    """the a2 units whose launch is predicted on a Winograd kernel"""
    return [p["unit"] for p in predict(dtype, N, H, W) if p["family"].startswith("wino-")]


# ---- tap buffers -----------------------------------------------------------------------------------------------------------
def taps_to_units(flat, offsets, dtype, N, H, W, upto=None):
    """flat: the tap buffer as a CPU uint8 tensor; offsets: 54 byte offsets -> the first `upto` (default all 54) tensors,
    NCHW float64 (exact)"""
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    es = 2 if dtype == "bf16" else 4
    out = []
    for off, (C, h, w) in list(zip(offsets, unit_shapes(N, H, W)))[:upto]:
        t = flat[off:off + N * h * w * C * es].view(tdt).view(N, h, w, C)
        out.append(t.permute(0, 3, 1, 2).double().contiguous())
    return out
