"""The parallel entropy stage on the MI355X: io_jpeg_decode_par_u8 (csrc/jpeg.hip, csrc/jpeg_sync.h) byte for byte against
the golden arrays and against io_jpeg_decode_u8, its info words against ``JpegImage.parallel_plan``, damaged streams, the
smallest inputs, its refusals, and ``jpeg.set_entropy("parallel")`` through the renderer."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_cases
from instaorder_amd import _lib, datasets, jpeg
from test_gpu_jpeg import FILL, MEAN, STD, _mixed_batch, offsets, upload
from test_gpu_jpeg import launch as launch_sequential

pytestmark = pytest.mark.gpu
NAMES, CASES, _ = jpeg_cases.load()
_plans = {}


def plan(im, key, size, max_rounds):
    """``parallel_plan`` of an image, computed once per (image, size, max_rounds)"""
    k = (key, size, max_rounds)
    if k not in _plans:
        _plans[k] = im.parallel_plan(size, max_rounds)
    return _plans[k]


def subsequences(im, size):
    return max(1, -(-im.nbytes_entropy // size))


def launch(t_pool, t_tables, t_desc, t_out, t_ws, t_status, size, max_rounds, t_info, **over):
    """io_jpeg_decode_par_u8 with device copies of the tables as given; ``over`` replaces single arguments of the call"""
    keep = [upload(t_pool), upload(t_tables), upload(np.frombuffer(t_desc, dtype=np.uint8))]
    a = dict(pool=keep[0].data_ptr(), pool_bytes=t_pool.size, tables_dev=keep[1].data_ptr(),
             tables_host=t_tables.ctypes.data_as(C.c_void_p), tables_bytes=t_tables.size, desc_dev=keep[2].data_ptr(),
             desc_host=C.cast(t_desc, C.c_void_p), n=len(t_desc), out=t_out.data_ptr(), out_bytes=t_out.numel(),
             ws=t_ws.data_ptr(), ws_bytes=t_ws.numel(), status=t_status.data_ptr(), size=size, max_rounds=max_rounds,
             info=t_info.data_ptr() if t_info is not None else 0)
    a.update(over)
    rc = _lib.lib().io_jpeg_decode_par_u8(C.c_void_p(a["pool"]), C.c_size_t(a["pool_bytes"]), C.c_void_p(a["tables_dev"]),
                                          a["tables_host"], C.c_size_t(a["tables_bytes"]), C.c_void_p(a["desc_dev"]),
                                          a["desc_host"], a["n"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]),
                                          C.c_void_p(a["ws"]), C.c_size_t(a["ws_bytes"]), C.c_void_p(a["status"]), a["size"],
                                          a["max_rounds"], C.c_void_p(a["info"]) if a["info"] else None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def par_workspace(desc, size):
    b = int(_lib.lib().io_jpeg_par_workspace_bytes(C.cast(desc, C.c_void_p), len(desc), size))
    assert b > 0, _lib.last_error()
    return b


@pytest.fixture(scope="module")
def all_cases():
    ims = [jpeg_cases.image(n) for n in NAMES]
    offs, total = offsets(ims)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    pool, tables, desc = jpeg.descriptors(ims, offs)
    expect = np.full(total, FILL, np.uint8)
    for name, o in zip(NAMES, offs):
        ref = CASES[name][1]
        expect[o:o + ref.size] = ref.reshape(-1)
    return ims, total, pool, tables, desc, expect


@pytest.mark.parametrize("size", [16, 24, 256])
def test_every_case_byte_exact_in_one_call(all_cases, size):
    """all 74 fixture files in ONE call, outputs at every alignment with guard bytes around them: the bytes of the golden
    arrays, status words zero, info words those of parallel_plan (every file converges and is clean with these rounds); the
    same once more on the used workspace; and with max_rounds = 2 the same bytes, bit 16 exactly where the plan says"""
    ims, total, pool, tables, desc, expect = all_cases
    rounds = max(subsequences(im, size) for im in ims)
    assert rounds <= 65535
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((par_workspace(desc, size),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    info = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    want = [plan(im, n, size, rounds) for im, n in zip(ims, NAMES)]
    assert all(p["fallback"] == 0 for p in want) and max(p["rounds"] for p in want) > 2
    for again in (0, 1):
        assert launch(pool, tables, desc, out, ws, status, size, rounds, info) == 0, _lib.last_error()
        assert status.cpu().numpy().tolist() == [0] * len(ims)
        assert info.cpu().numpy().tolist() == [p["rounds"] for p in want]
        got = out.cpu().numpy()
        for name, im, d in zip(NAMES, ims, desc):
            ref = CASES[name][1]
            g = got[d.out_off:d.out_off + ref.size].reshape(ref.shape)
            assert np.array_equal(g, ref), "%s: %d of %d bytes differ" % (name, (g != ref).sum(), ref.size)
        assert np.array_equal(got, expect), "a guard byte was written"
        out.fill_(FILL)
        status.fill_(-1)
        info.fill_(-1)
    two = [plan(im, n, size, 2) for im, n in zip(ims, NAMES)]
    assert any(p["fallback"] == 1 << 16 for p in two) and any(p["fallback"] == 0 for p in two)
    assert launch(pool, tables, desc, out, ws, status, size, 2, info) == 0, _lib.last_error()
    assert status.cpu().numpy().tolist() == [0] * len(ims)
    assert info.cpu().numpy().tolist() == [p["rounds"] | p["fallback"] for p in two]
    assert np.array_equal(out.cpu().numpy(), expect)
    out.fill_(FILL)
    assert launch(pool, tables, desc, out, ws, status, size, 2, None) == 0, _lib.last_error()      # no info words wanted
    assert np.array_equal(out.cpu().numpy(), expect)


@pytest.mark.parametrize("size", [16, 256])
def test_damaged_streams_fall_back_and_equal_the_sequential_stage(size):
    """the truncations and mutations of tests/test_gpu_jpeg.py between intact images in one call: the status words are
    those of ``status_of``, bit 17 is set for exactly the streams that do not decode, the info words are the plan's, and
    every pixel -- of the damaged images too -- is what io_jpeg_decode_u8 writes for the same batch"""
    ims, want = [], []
    for s, name in enumerate(jpeg_cases.FUZZ):
        base = jpeg_cases.image(name)
        ent = base.entropy_bytes()
        alts = [base.with_entropy(ent[:len(ent) // 3], name + " cut at a third"), base.with_entropy(ent[:-1], name + " cut by one"),
                base.with_entropy(b"", name + " empty")]
        alts += [base.with_entropy(jpeg_cases.mutated(ent, m), "%s mutation %d" % (name, m)) for m in range(4 * s, 4 * s + 4)]
        for alt in alts:
            ims += [base, alt]
            want += [0, jpeg_cases.status_of(alt)[0]]
    assert sum(1 for w in want if w) >= 9 and len(set(want)) >= 3
    rounds = max(subsequences(im, size) for im in ims)
    plans = [plan(im, im.name, size, rounds) for im in ims]
    offs, total = offsets(ims)
    pool, tables, desc = jpeg.descriptors(ims, offs)
    ref = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.empty(par_workspace(desc, size), dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert launch_sequential(pool, tables, desc, ref, ws, status) == 0, _lib.last_error()
    assert status.cpu().numpy().tolist() == want
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    status.fill_(-1)
    info = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert launch(pool, tables, desc, out, ws, status, size, rounds, info) == 0, _lib.last_error()
    assert status.cpu().numpy().tolist() == want
    words = info.cpu().numpy().tolist()
    assert [w >> 16 for w in words] == [2 if st else 0 for st in want]
    assert words == [p["rounds"] | p["fallback"] for p in plans]
    assert torch.equal(out, ref)
    keep = jpeg.get_entropy()
    try:
        jpeg.set_entropy("parallel", size, rounds)
        bad = next(im for im, w in zip(ims, want) if w)
        with pytest.raises(RuntimeError, match="cut at a third"):
            jpeg.decode([ims[0], bad, ims[0]], "cuda")
    finally:
        jpeg.set_entropy(keep["mode"], keep["subseq_bytes"], keep["max_rounds"])


def test_smallest_inputs_alone_in_a_batch():
    """a 1 x 1 file, and a stream of two bytes (one subsequence, which cannot hold the image), each alone in a call"""
    one = jpeg_cases.image("1x1_420_q85")
    two = jpeg_cases.image("9x17_420_q85")
    two = two.with_entropy(two.entropy_bytes()[:2], "two bytes")
    for im, size in ((one, 16), (one, 4096), (two, 16), (two, 256)):
        offs, total = offsets([im])
        pool, tables, desc = jpeg.descriptors([im], offs)
        out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        ref = out.clone()
        ws = torch.full((par_workspace(desc, size),), FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        assert launch(pool, tables, desc, out, ws, status, size, 64, info) == 0, _lib.last_error()
        p = im.parallel_plan(size, 64)
        assert p["subsequences"] == 1 and p["rounds"] == 1
        st = jpeg_cases.status_of(im)[0]
        assert status.item() == st and info.item() == 1 | p["fallback"] and p["fallback"] == (1 << 17 if st else 0)
        status.fill_(-1)
        assert launch_sequential(pool, tables, desc, ref, ws, status) == 0 and status.item() == st
        assert torch.equal(out, ref) and bool((out[:offs[0]] == FILL).all())
        if st == 0:
            assert np.array_equal(out[offs[0]:offs[0] + 3].cpu().numpy(), CASES["1x1_420_q85"][1].reshape(-1))
    assert jpeg_cases.status_of(two)[0] != 0


def test_refusals_leave_every_buffer_untouched():
    ims = [jpeg_cases.image(n) for n in ("9x17_420_q85", "21x35_444_rst2")]
    sizes = [im.H * im.W * 3 for im in ims]
    pool, tables, desc = jpeg.descriptors(ims, [16, 1024])
    out = torch.full((1024 + sizes[1],), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((par_workspace(desc, 16),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(size=16, max_rounds=8, d=None, **over):
        dd = (_lib.JpegDesc * 2)()
        C.memmove(dd, desc, C.sizeof(desc))
        for k, v in (d or {}).items():
            setattr(dd[0], k, v)
        return launch(pool, tables, dd, out, ws, status, size, max_rounds, info, **over)

    L.io_prof_begin_ex(0)
    for size in (8, 20, 8192, 0, -16):
        assert call(size=size) == -1 and "subseq_bytes" in _lib.last_error(), size
    for r in (0, -1, 65536):
        assert call(max_rounds=r) == -1 and "max_rounds" in _lib.last_error(), r
    assert call(ws_bytes=ws.numel() - 1) == -2 and "workspace" in _lib.last_error()
    assert call(ws_bytes=jpeg.workspace_bytes(desc, "sequential")) == -2          # the sequential stage's size is too small
    assert call(size=24, ws_bytes=par_workspace(desc, 24) - 1) == -2
    for kw, why in ((dict(d=dict(hs=4)), "sampling"), (dict(d=dict(H=0)), "size"), (dict(d=dict(data_off=-1)), "data range"),
                    (dict(d=dict(data_bytes=pool.size + 1)), "byte pool"), (dict(out_bytes=1024 + sizes[1] - 1), "output"),
                    (dict(n=0), "empty"), (dict(ws=ws.data_ptr() + 4), "aligned"), (dict(out=0), "null"),
                    (dict(status=0), "null"), (dict(tables_host=None), "null")):
        assert call(**kw) == -1 and why in _lib.last_error(), (why, _lib.last_error())
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all()) and bool((status == -1).all()) and bool((info == -1).all())
    assert call() == 0, _lib.last_error()
    got = out.cpu().numpy()
    for (o, n), name in zip(((16, sizes[0]), (1024, sizes[1])), ("9x17_420_q85", "21x35_444_rst2")):
        assert np.array_equal(got[o:o + n], CASES[name][1].reshape(-1))
    assert (got[:16] == FILL).all() and (got[16 + sizes[0]:1024] == FILL).all()
    assert status.cpu().numpy().tolist() == [0, 0] and bool((info >= 1).all())


def test_decode_and_the_renderer_follow_set_entropy():
    """jpeg.decode(entropy=..., info=True), and a PairRenderer batch that mixes arrays and JpegImages under
    set_entropy("parallel") against the sequential setting, bit for bit; a broken file is still reported"""
    names = ["33x47_420_q85", "1x1_gray_q85", "21x35_422_rst2", "160x208_420_q90"]
    ims = [jpeg_cases.image(n) for n in names]
    got, words = jpeg.decode(ims, "cuda", entropy="parallel", info=True)
    for g, n in zip(got, names):
        assert np.array_equal(g.cpu().numpy(), CASES[n][1]), n
    e = jpeg.get_entropy()
    assert e["mode"] == "sequential"
    assert words.tolist() == [p["rounds"] | p["fallback"] for p in (im.parallel_plan(e["subseq_bytes"], e["max_rounds"]) for im in ims)]
    assert not jpeg.decode(ims, "cuda", info=True)[1].any()                       # the sequential stage has no info words
    S = 64
    arrays, jp, masks, enc, items = _mixed_batch()
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(jp, enc, items)]
    assert np.abs(want[0]).max() > 0
    try:
        for size, rounds in ((256, 64), (16, 2), (24, 400)):
            jpeg.set_entropy("parallel", size, rounds)
            r = datasets.PairRenderer(S, MEAN, STD)
            for name, ii, mm in (("jpeg + dense masks", jp, masks), ("jpeg + encoded masks", jp, enc)):
                for g, w, plane in zip(r.render(ii, mm, items), want, ("rgb", "modal1", "modal2")):
                    assert np.array_equal(g.cpu().numpy(), w), (size, name, plane)
            r.check_status()
            broken = jp[0].with_entropy(jp[0].entropy_bytes()[:40], "broken.jpg")
            r.render([broken, jp[1], arrays[2]], enc, items)
            with pytest.raises(RuntimeError, match="broken.jpg"):
                r.check_status()
    finally:
        jpeg.set_entropy(e["mode"], e["subseq_bytes"], e["max_rounds"])
