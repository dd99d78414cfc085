"""Gradient clipping without a GPU: the C ABI additions, validation of ``max_grad_norm``, the segment layout handed to the
optimisers, and checkpoint layout with and without clipping."""
import ctypes as C
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from instaorder_amd import _lib  # noqa: E402
from instaorder_amd.optim import FlatAdam, FlatSGD, FusedAdam, FusedSGD  # noqa: E402

FUNCS = {"io_grad_norm": 10, "io_grad_norm_workspace_bytes": 2, "io_sgd_momentum_clipped": 9, "io_adam_step_clipped": 14}


def _header():
    return open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()


def test_clip_abi_declared_typed_and_exported():
    hdr = _header()
    for name, nargs in FUNCS.items():
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        if name != "io_grad_norm_workspace_bytes":
            assert args[-1].startswith("hipStream_t")
    # the clipped updates: the existing argument lists, then the record, then the stream
    for plain, clipped in (("io_sgd_momentum", "io_sgd_momentum_clipped"), ("io_adam_step", "io_adam_step_clipped")):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[clipped][1]
        assert b[:len(a) - 1] == a[:-1] and b[-2:] == [C.c_void_p, C.c_void_p]
        decl = re.search(r"int %s\(([^;]*)\);" % clipped, hdr).group(1)
        assert "const io_clip_state* clip, hipStream_t stream" in " ".join(decl.split())
    assert re.search(r"typedef struct io_clip_state \{[^}]*\} io_clip_state;", hdr), "io_clip_state is not declared"
    if os.path.isfile(_lib.LIB_PATH):
        lib = _lib.lib()
        for name in FUNCS:
            assert hasattr(lib, name), name
        assert lib.io_abi_version() == 1


def test_clip_state_record_layout():
    """64 bytes, the fields in the header's order (the ctypes mirror is what grad_stats() decodes)."""
    body = re.search(r"typedef struct io_clip_state \{([^}]*)\}", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[.*", "", f.split()[-1]) for f in body.split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.ClipState._fields_]
    assert C.sizeof(_lib.ClipState) == 64
    assert _lib.ClipState.steps.offset == 16 and _lib.ClipState.skipped.offset == 32


def test_workspace_bytes_and_chunk():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    ch = lib.io_grad_norm_chunk_floats()
    assert ch > 0 and ch % 1024 == 0
    # one fp64 slot per chunk, plus one partial chunk per segment at the most
    assert lib.io_grad_norm_workspace_bytes(ch, 1) == 8 * 2
    assert lib.io_grad_norm_workspace_bytes(3 * ch + 12, 16) == 8 * (4 + 16)
    assert lib.io_grad_norm_workspace_bytes(0, 1) == 8


def test_grad_norm_refuses_bad_segments_before_any_launch():
    """The argument checks run on the host, in front of the launches: they answer without a device."""
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()

    def call(n, offs, max_norm=1.0, nseg=None):
        arr = (C.c_size_t * len(offs))(*offs)
        return lib.io_grad_norm(None, n, arr, len(offs) - 1 if nseg is None else nseg, max_norm, None, 0, None, None, None)
    for n, offs in ((64, [0, 30, 64]), (64, [4, 64]), (64, [0, 60]), (64, [0, 40, 32, 64])):
        assert call(n, offs) != 0, offs
        assert "grad_norm" in _lib.last_error()
    assert call(64, [0] * 18, nseg=17) != 0 and "nseg" in _lib.last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert call(64, [0, 64], max_norm=bad) != 0 and "max_norm" in _lib.last_error()


class _Tiny(nn.Module):
    def __init__(self):
        super(_Tiny, self).__init__()
        self.a = nn.Linear(5, 7)
        self.b = nn.Conv2d(3, 4, 3)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), "1.0", True])
@pytest.mark.parametrize("cls", [FlatSGD, FlatAdam, FusedSGD, FusedAdam])
def test_max_grad_norm_is_validated(cls, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        cls(_Tiny(), lr=1e-3, max_grad_norm=bad)


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdam])
@pytest.mark.parametrize("clip", [None, 1.0, float("inf")])
def test_fused_optimisers_still_need_the_flat_resnet(cls, clip):
    with pytest.raises(TypeError, match="flat parameter buffer"):
        cls(_Tiny(), lr=1e-3, max_grad_norm=clip)


@pytest.mark.parametrize("cls", [FlatSGD, FlatAdam])
def test_state_dict_layout_is_the_same_with_and_without_clipping(cls):
    torch.manual_seed(0)
    opts = [cls(_Tiny(), lr=1e-3, max_grad_norm=c) for c in (None, 2.5, float("inf"))]
    assert [o.max_grad_norm for o in opts] == [None, 2.5, float("inf")]
    sds = [o.state_dict() for o in opts]
    ref = (torch.optim.SGD if cls is FlatSGD else torch.optim.Adam)
    kw = dict(momentum=0.9) if cls is FlatSGD else {}
    torch_keys = set(ref(_Tiny().parameters(), lr=1e-3, **kw).state_dict()["param_groups"][0])
    for sd in sds:
        assert list(sd) == ["state", "param_groups"] and len(sd["param_groups"]) == 1
        # nothing about clipping in torch's layout (FlatSGD writes the subset of torch.optim.SGD's keys it honours)
        keys = set(sd["param_groups"][0])
        assert keys == torch_keys if cls is FlatAdam else (keys <= torch_keys and "momentum" in keys)
        assert sd["param_groups"][0] == sds[0]["param_groups"][0]
        assert set(sd["state"]) == set(sds[0]["state"])
        for i in sd["state"]:
            assert set(sd["state"][i]) == set(sds[0]["state"][i])
    # ... and they load into each other and into torch's own optimiser
    opts[0].load_state_dict(sds[1])
    opts[1].load_state_dict(sds[0])
    assert opts[0].max_grad_norm is None and opts[1].max_grad_norm == 2.5
    ref(_Tiny().parameters(), lr=1.0, **kw).load_state_dict(sds[1])


def test_fused_state_dict_layout_with_clipping():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    from instaorder_amd import resnet_cls
    net = resnet_cls.resnet50_cls(in_channels=5, num_classes=2)
    for cls in (FusedSGD, FusedAdam):
        a, b = cls(net, lr=1e-3).state_dict(), cls(net, lr=1e-3, max_grad_norm=1.0).state_dict()
        assert a["param_groups"] == b["param_groups"] and set(a["state"]) == set(b["state"])


def test_segments_must_tile_the_buffer():
    opt = FlatSGD(_Tiny(), lr=1e-3, max_grad_norm=1.0)
    n = opt.flat_grads.numel()
    assert n % 64 == 0 and opt.clip_state is None
    opt.set_grad_segments([(64, n), (0, 64)], ("late", "early"))           # execution order: back to front
    assert opt._seg_offsets == [0, 64, n] and opt._seg_names == ("early", "late")
    for bad in ([(0, 64)] * 17, [(0, 62), (62, n)], [(64, n)], [(0, 64), (128, n)], [(0, 128), (64, n)]):
        with pytest.raises(ValueError, match="segments"):
            opt.set_grad_segments(bad)
    with pytest.raises(ValueError, match="segments"):
        opt.set_grad_segments([(0, 64), (64, n)], ("x", "x"))
    with pytest.raises(RuntimeError, match="no clipped step"):
        opt.grad_stats()


def _cfg(**kw):
    cfg = dict(algo="InstaOrderNet_o", lr=1e-3, weight_decay=1e-4, optim="SGD", beta1=0.5, backbone_arch="resnet50_cls",
               backbone_param=dict(in_channels=5, num_classes=2))
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("optim", ["SGD", "Adam"])
def test_single_stage_model_passes_clip_grad_norm(optim):
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    if torch.cuda.is_available():
        pytest.skip("constructs on the CPU")
    from instaorder_amd.single_stage_model import SingleStageModel
    off = SingleStageModel(_cfg(optim=optim))
    assert off.optim.max_grad_norm is None and off.optim._seg_offsets is None
    m = SingleStageModel(_cfg(optim=optim, clip_grad_norm=0.5))
    assert m.optim.max_grad_norm == 0.5
    # the four backward stages of the ResNet, ascending in the buffer: layer1 + stem first
    assert m.optim._seg_names == ("layer1+stem", "layer2", "layer3", "heads+layer4")
    assert m.optim._seg_offsets[0] == 0 and m.optim._seg_offsets[-1] == m.net.flat_grads.numel()
    assert m.optim.state_dict()["param_groups"] == off.optim.state_dict()["param_groups"]
    with pytest.raises(ValueError, match="max_grad_norm"):
        SingleStageModel(_cfg(optim=optim, clip_grad_norm=-1.0))


def test_single_stage_model_clip_segments_midas():
    if torch.cuda.is_available():
        pytest.skip("constructs on the CPU")
    import instaorder_amd as ia
    cfg = dict(algo="InstaDepthNet_d", lr=1e-4, weight_decay=1e-4, optim="Adam", beta1=0.9, pretrained_weight=None,
               clip_grad_norm=float("inf"))
    m = ia.InstaDepthNet_d(cfg, dist_model=False)
    assert isinstance(m.optim, FlatAdam) and m.optim.max_grad_norm == float("inf")
    assert sorted(m.optim._seg_names) == sorted(m.STAGE_NAMES)
    assert m.optim._seg_names[-1] == m.STAGE_NAMES[0]               # everything behind the encoder lies last in the buffer
    assert m.optim._seg_offsets[-1] == m.optim.flat_grads.numel()
