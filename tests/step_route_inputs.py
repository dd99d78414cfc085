"""The per-block route rules of the ResNet-50 training step, restated in Python from the host code of csrc/net.hip and
csrc/conv_p256.hip AS IT STOOD BEFORE the route table (each rule cites the function and the lines it restates in that
revision: the one before the change that added this file).  tests/test_step_routes_cpu.py holds the table
io_net_step_routes returns to these rules, so the table cannot drift from what the executor did when every route was
decided inline.  No GPU, no library: plain integers."""
import itertools

F32, BF16 = 0, 1
K_MAX_GROUPS = 8            # net.hip:18
TILE = 128                  # kIoStatTileRows, io_common.h:255
XB_BF16_MAXP = 64           # IO_XB_BF16_MAXP, net.hip:407-409 (IO_XB_BF16_L1 = 1, :410-412)
XOP_MAX_CI = 2048           # kXopMaxCi, conv_p256.hip:73

# io_net_create, net.hip:988-997: Bottleneck x [3, 4, 6, 3], stride 2 on the first block of layers 2-4, which (with layer 1's)
# also has the downsample branch
BLOCKS = [(planes, 2 if (bi == 0 and li > 0) else 1, bi == 0)
          for li, (n, planes) in enumerate(zip((3, 4, 6, 3), (64, 128, 256, 512))) for bi in range(n)]

# the case set of tests/test_step_routes_cpu.py: every combination with G | N
DTYPES = (F32, BF16)
SHAPES = ((4, 64), (3, 96), (16, 128), (32, 256), (256, 256))
GROUPS = (1, 2, 8)
P256_MODES = (0, 1, 3)
XOPS = (0, 1)
NCUS = (256, 64)


def cases():
    for dt, (N, S), G, mode, xop, ncu in itertools.product(DTYPES, SHAPES, GROUPS, P256_MODES, XOPS, NCUS):
        if N % G == 0:
            yield dt, N, S, G, mode, xop, ncu


def tiles_ok(M, G):
    """net.hip:670 tiles_ok (== the inline tests of xr_route :427 and fuse_in :445)"""
    return M % G == 0 and (M // G) % TILE == 0


def rounds_ok(tiles, mode, ncu):
    """conv_p256.hip:542-546 p256_rounds_ok"""
    rounds = (tiles + ncu - 1) // ncu
    return mode == 3 or tiles * 10 >= rounds * ncu * 8


def takes_xop(M, Ci, Co, Mg, mode, xop, ncu):
    """conv_p256.hip:570-575 io_conv_p256_takes_xop, the hand-written shape part of the launcher's refusals"""
    if not mode or not xop:
        return False
    if M % 256 or Ci % 64 or Ci > XOP_MAX_CI or Co % 128 or Mg <= 0 or Mg % 256 or M % Mg:
        return False
    if 256.0 * Ci * 2.0 >= 4.0e9 or 256.0 * Co * 2.0 >= 4.0e9:
        return False
    return rounds_ok(M // 256 * (Co // (256 if Co % 256 == 0 else 128)), mode, ncu)


FIELDS = ("tiles_in", "tiles_out", "f2", "f3", "bits_written", "x3", "x3p", "x1d", "x1s", "carry", "have_tiles",
          "a1_stored", "a2_stored", "bits_alloc")


def routes(dt, N, S, G, mode, xop, ncu):
    """-> one dict per block: FIELDS (bool), out_route (0 | 1 | 2), stage (0..3)"""
    nb = len(BLOCKS)
    rows = []
    H = S // 4                                                       # run_forward, net.hip:542, 554
    res = -1
    for i, (planes, stride, down) in enumerate(BLOCKS):
        Ho = H // stride                                             # :562
        Min, Mout = N * H * H, N * Ho * Ho                           # :563
        r = dict(tiles_in=tiles_ok(Min, G), tiles_out=tiles_ok(Mout, G))
        # make_plan, net.hip:181-194 (storage; depends on neither G nor a switch)
        never = dt == F32 and Mout % K_MAX_GROUPS == 0 and (Mout // K_MAX_GROUPS) % TILE == 0
        r["a1_stored"] = not (never and stride == 1)                 # :183
        r["a2_stored"] = not never                                   # :185
        r["bits_alloc"] = dt == BF16 and Mout % 256 == 0             # :194
        # fuse_in, net.hip:444-446; run_forward :576
        r["f3"] = dt == F32 and tiles_ok(Mout, G)
        r["f2"] = r["f3"] and stride == 1
        # xr_route, net.hip:423-431
        if i + 1 >= nb or not tiles_ok(Mout, G):
            r["out_route"] = 0
        elif dt == F32 or planes <= XB_BF16_MAXP:
            r["out_route"] = 1
        else:
            r["out_route"] = 2 if takes_xop(Mout, planes * 4, BLOCKS[i + 1][0], Mout // G, mode, xop, ncu) else 0
        r["bits_written"] = r["bits_alloc"] and r["out_route"] != 1  # bits_written, net.hip:440-442
        # run_backward, net.hip:828-838
        r["x3p"] = (dt == BF16 and planes > XB_BF16_MAXP and tiles_ok(Mout, G) and
                    takes_xop(Mout, planes * 4, planes, Mout // G, mode, xop, ncu))
        r["x3"] = ((dt == F32 and tiles_ok(Mout, G)) or r["x3p"] or
                   (dt == BF16 and planes <= XB_BF16_MAXP and tiles_ok(Mout, G)))
        r["x1d"] = stride == 1 and dt == F32 and tiles_ok(Min, G) and tiles_ok(Mout, G)
        r["x1s"] = stride != 1 and dt == F32 and tiles_ok(Min, G) and r["a1_stored"]
        r["carry"] = i > 0 and tiles_ok(Min, G)                      # :893
        # stage_of, net.hip:788-798: a stride-2 block opens a resolution; numbered from the back below
        if i == 0 or stride != 1:
            res += 1
        r["stage"] = res
        rows.append(r)
        H = Ho
    for i, r in enumerate(rows):
        r["stage"] = res - r["stage"]
        # the running have_tiles of run_backward (:799, :846, :901; :807 in a skipped stage): false at the last block, then
        # what the block BEHIND this one (processed just before it) left as its `carry`
        r["have_tiles"] = i + 1 < nb and rows[i + 1]["carry"]
    return rows


# bit positions of io_net_step_routes' words (include/instaorder_hip.h)
BITS = dict(tiles_in=2, tiles_out=3, f2=4, f3=5, bits_written=6, x3=7, x3p=8, x1d=9, x1s=10, carry=11, have_tiles=12,
            a1_stored=13, a2_stored=14, bits_alloc=15)


def pack(r):
    w = r["out_route"] | (r["stage"] << 16)
    for k, b in BITS.items():
        w |= int(bool(r[k])) << b
    return w


def unpack(w):
    r = {k: bool((w >> b) & 1) for k, b in BITS.items()}
    r["out_route"], r["stage"] = w & 3, (w >> 16) & 3
    return r
