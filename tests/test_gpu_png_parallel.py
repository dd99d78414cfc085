"""The parallel inflate stage on the MI355X: io_png_decode_par (csrc/png.hip, csrc/png_inflate_par.h) byte for byte against
the expected arrays, info words against ``PngImage.parallel_plan``, damaged streams against io_png_decode in the same
test, the entry point's refusals, and the renderer and ``png.decode`` under ``png.set_inflate("parallel")``."""
import ctypes as C

import numpy as np
import pytest
import torch

import png_cases
import png_parallel_cases as cases
from instaorder_amd import _lib, datasets, png
from test_gpu_png import FILL, MEAN, STD, _as_png, offsets, upload
from test_gpu_png import launch as launch_sequential
from test_gpu_jpeg import _mixed_batch

pytestmark = pytest.mark.gpu
CHUNKS = cases.CHUNKS


def launch(t_pool, t_desc, t_out, t_ws, t_status, chunk_bytes, t_info, **over):
    """io_png_decode_par with device copies of the tables as given; ``over`` replaces single arguments of the call"""
    keep = [upload(t_pool), upload(over.pop("desc_dev_table", t_desc))]
    a = dict(pool=keep[0].data_ptr(), pool_bytes=t_pool.size, desc_dev=keep[1].data_ptr(), desc_host=C.cast(t_desc, C.c_void_p),
             n=len(t_desc), out=t_out.data_ptr(), out_bytes=t_out.numel(), ws=t_ws.data_ptr(), ws_bytes=t_ws.numel(),
             status=t_status.data_ptr(), chunk_bytes=chunk_bytes, info=None if t_info is None else t_info.data_ptr())
    a.update(over)
    rc = _lib.lib().io_png_decode_par(C.c_void_p(a["pool"]), C.c_size_t(a["pool_bytes"]), C.c_void_p(a["desc_dev"]),
                                      a["desc_host"], a["n"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]),
                                      C.c_void_p(a["ws"]), C.c_size_t(a["ws_bytes"]), C.c_void_p(a["status"]), a["chunk_bytes"],
                                      C.c_void_p(a["info"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def run(ims, chunk_bytes, with_info=True):
    """one io_png_decode_par call: (offsets, total, output bytes, status words, info words)"""
    offs, total = offsets(ims)
    pool, desc = png.descriptors(ims, offs)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    need = png.workspace_bytes(desc, dict(mode="parallel", chunk_bytes=chunk_bytes))
    ws = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    info = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda") if with_info else None
    assert launch(pool, desc, out, ws, status, chunk_bytes, info) == 0, _lib.last_error()
    return offs, total, out.cpu().numpy(), status.cpu().numpy().tolist(), info.cpu().numpy().tolist() if with_info else None


@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_decode_par_byte_exact_in_one_call(chunk_bytes):
    """ONE call over every image of stream_cases(), batch_cases() and the property streams: bytes equal to the expected
    arrays, all status words zero, info words those of ``parallel_plan``, bytes outside the slots untouched; the same call
    again gives the same words and bytes, and so does a call without info words."""
    pairs = cases.intact_cases()
    ims = [im for im, _ in pairs]
    plans = [cases.plan(im, chunk_bytes) for im in ims]
    assert sum(p["parallel"] for p in plans) >= 8 and any(len(p["chain"]) >= 8 for p in plans)      # both paths in one call
    assert sum(not p["parallel"] for p in plans) >= 8
    offs, total, got, status, info = run(ims, chunk_bytes)
    assert status == [0] * len(ims), [(im.name, s) for im, s in zip(ims, status) if s]
    assert info == [p["info"] for p in plans], [(im.name, hex(i), hex(p["info"])) for im, i, p in zip(ims, info, plans)
                                                if i != p["info"]]
    expect = np.full(total, FILL, np.uint8)
    for (im, want), o in zip(pairs, offs):
        ref = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
        g = got[o:o + ref.size]
        assert np.array_equal(g, ref), "%s: %d of %d bytes differ" % (im.name, (g != ref).sum(), ref.size)
        expect[o:o + ref.size] = ref
    assert np.array_equal(got, expect), "a guard byte was written"
    again = run(ims, chunk_bytes)
    assert again[3] == status and again[4] == info and np.array_equal(again[2], got)
    blind = run(ims, chunk_bytes, with_info=False)
    assert blind[3] == status and np.array_equal(blind[2], got)


def test_damaged_streams_equal_the_sequential_entry_point():
    """``damaged()`` and the damaged long-chain stream, every one behind an intact image that decodes in parallel, in one
    call per chunk size: status words and slots equal those of io_png_decode on the same inputs, the info words are the
    plan's, and the neighbours decode."""
    good = cases.property_cases()[0][0]
    ims = []
    for label, im in cases.damaged_cases():
        ims += [good, im]
    offs, total = offsets(ims)
    pool, desc = png.descriptors(ims, offs)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((png.workspace_bytes(desc, "sequential"),), FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert launch_sequential(pool, desc, out, ws, st) == 0, _lib.last_error()
    want, want_status = out.cpu().numpy(), st.cpu().numpy().tolist()
    assert set(want_status) == set(range(10))
    ref = good.to_host().reshape(-1)
    for cb in CHUNKS:
        o2, t2, got, status, info = run(ims, cb)
        assert (o2, t2) == (offs, total)
        assert status == want_status, [(im.name, s, w) for im, s, w in zip(ims, status, want_status) if s != w][:5]
        assert info == [cases.plan(im, cb)["info"] for im in ims]
        assert sum(1 for i, s in zip(info, status) if i >> 16 == 0 and s == 8) >= 10    # Adler-32 behind a parallel decode
        covered = np.zeros(total, bool)
        for im, o, s in zip(ims, offs, status):
            covered[o:o + im.out_bytes] = True
            if s == 0:
                assert np.array_equal(got[o:o + im.out_bytes], want[o:o + im.out_bytes]), im.name
            if im is good:
                assert s == 0 and np.array_equal(got[o:o + ref.size], ref)
        assert (got[~covered] == FILL).all(), "a guard byte was written"


def test_entry_point_refusals_launch_nothing():
    ims = [cases.property_cases()[0][0], png_cases.build(6, 7, "gray16", "mix")[0]]
    sizes = [im.out_bytes for im in ims]
    second = (17 + sizes[0] + 63) // 64 * 64
    pool, desc0 = png.descriptors(ims, [17, second])
    out = torch.full((second + sizes[1],), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((png.workspace_bytes(desc0, dict(mode="parallel", chunk_bytes=256)),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(d=None, which=0, chunk_bytes=256, **over):
        desc = (_lib.PngDesc * 2)()
        C.memmove(desc, desc0, C.sizeof(desc0))
        for k, v in (d or {}).items():
            setattr(desc[which], k, v)
        return launch(pool, desc, out, ws, status, chunk_bytes, info, desc_dev_table=desc0, **over)

    L.io_prof_begin_ex(0)
    refused = [
        (call(chunk_bytes=0), "chunk_bytes"), (call(chunk_bytes=128), "chunk_bytes"), (call(chunk_bytes=300), "chunk_bytes"),
        (call(chunk_bytes=-256), "chunk_bytes"), (call(chunk_bytes=(1 << 20) + 256), "chunk_bytes"),
        (call(dict(H=0)), "size"), (call(dict(W=65536)), "size"), (call(dict(channels=2)), "channels"),
        (call(dict(depth=16)), "channels"), (call(dict(data_bytes=-5)), "data range"),
        (call(dict(data_bytes=desc0[1].data_bytes + 1), which=1), "byte pool"), (call(pool_bytes=pool.size - 1), "byte pool"),
        (call(dict(out_off=-1)), "output"), (call(out_bytes=second + sizes[1] - 1), "output"),
        (call(dict(out_off=second - 1), which=1), "2-byte aligned"),
        (call(n=0), "empty"), (call(n=65536), "65535"), (call(ws=ws.data_ptr() + 4), "aligned"),
        (call(out=0), "null"), (call(ws=0), "null"), (call(pool=0), "null"), (call(status=0), "null"), (call(desc_dev=0), "null"),
    ]
    for k, (rc, _) in enumerate(refused):
        assert rc == -1, (k, rc)
    assert call(desc_host=None) == -1
    assert call(chunk_bytes=300) == -1 and "chunk_bytes" in _lib.last_error()
    assert call(ws_bytes=ws.numel() - 1) == -2 and "workspace" in _lib.last_error()        # IO_ERR_WORKSPACE
    assert call(ws_bytes=png.workspace_bytes(desc0, "sequential")) == -2                    # the sequential size is too small
    assert call(dict(channels=2)) == -1 and "channels" in _lib.last_error()
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all()) and bool((status == -1).all()) and bool((info == -1).all())
    assert call() == 0, _lib.last_error()                       # and the tables as they are decode
    got = out.cpu().numpy()
    for (o, n), im in zip(((17, sizes[0]), (second, sizes[1])), ims):
        assert np.array_equal(got[o:o + n], im.to_host().reshape(-1).view(np.uint8))
    assert (got[:17] == FILL).all() and (got[17 + sizes[0]:second] == FILL).all()
    assert status.cpu().numpy().tolist() == [0, 0]
    assert info.cpu().numpy().tolist() == [cases.plan(im, 256)["info"] for im in ims]


def test_renderer_and_decode_follow_the_setting():
    """one small mixed batch through the renderer under ``png.set_inflate("parallel", 256)``: the batch of the sequential
    setting bit for bit (files whose chains have several chunks among them); ``png.decode(inflate="parallel", info=True)``
    on pictures and on a raw16 map."""
    S = 64
    arrays, jp, masks, enc, items = _mixed_batch()
    # pictures of the batch's shapes (its own arrays are noise, which zlib stores: chains of one) in small dynamic blocks
    pg = [_as_png(png_cases.picture(a.shape[0], a.shape[1], "rgb", seed=40 + k), "image%d.png" % k, mem_level=1)
          for k, a in enumerate(arrays)]
    depth, depth_want = png_cases.build(70, 90, "gray16", "mix", seed=31, mem_level=1, name="depth.png")
    assert png.get_inflate()["mode"] == "sequential"
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render([pg[0], jp[1], pg[2]], enc, items)]
    plain = [t.cpu().numpy() for t in png.decode(pg + [depth], "cuda")]
    try:
        png.set_inflate("parallel", 256)
        r = datasets.PairRenderer(S, MEAN, STD)
        got = r.render([pg[0], jp[1], pg[2]], enc, items)
        for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
            assert np.array_equal(g.cpu().numpy(), w), plane
        r.check_status()
        tensors, info = png.decode(pg + [depth], "cuda", info=True)
    finally:
        png.set_inflate("sequential")
    assert info.dtype == np.int32 and info.tolist() == [im.parallel_plan(256)["info"] for im in pg + [depth]]
    assert all(i >> 16 == 0 and i >= 2 for i in info), [hex(i) for i in info]      # every one of them decoded in parallel
    for t, w in zip(tensors, plain):
        assert np.array_equal(t.cpu().numpy(), w)
    assert tensors[-1].dtype == torch.uint16 and np.array_equal(tensors[-1].cpu().numpy(), depth_want)
    tensors, info2 = png.decode([depth], "cuda", inflate="parallel", info=True)      # the per-call override, default chunk size
    assert np.array_equal(tensors[0].cpu().numpy(), depth_want)
    assert info2.tolist() == [depth.parallel_plan(png.DEFAULT_CHUNK_BYTES)["info"]]
    with pytest.raises(ValueError, match="info words"):
        png.decode([depth], "cuda", info=True)
    res, st, ims, words = png.decode([depth], "cuda", check=False, inflate="parallel", info=True)
    assert st.cpu().numpy().tolist() == [0] and words.cpu().numpy().tolist() == info2.tolist() and ims == [depth]
