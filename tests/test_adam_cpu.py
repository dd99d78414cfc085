"""optim: Adam without a GPU: the C ABI entry point, checkpoint interchange of FlatAdam / FusedAdam with torch.optim.Adam,
SingleStageModel's config handling, the launch plan over live / gradient-less parameters, and the Adam kernel's gfx950
assembly under tools/scan_store_hazard.py."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from instaorder_amd import _lib  # noqa: E402
from instaorder_amd.optim import FlatAdam, FusedAdam, _AdamFlat  # noqa: E402


def test_io_adam_step_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    decl = re.search(r"int io_adam_step\(([^;]*)\);", hdr)
    assert decl, "io_adam_step is not declared in include/instaorder_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 13 and args[4].startswith("size_t") and args[-1].startswith("hipStream_t")
    res, argtypes = _lib.SIGNATURES["io_adam_step"]
    assert len(argtypes) == len(args)
    if os.path.isfile(_lib.LIB_PATH):
        assert hasattr(_lib.lib(), "io_adam_step")
        assert _lib.lib().io_abi_version() == 1


class _Tiny(nn.Module):
    def __init__(self):
        super(_Tiny, self).__init__()
        self.a = nn.Linear(5, 7)
        self.b = nn.Conv2d(3, 4, 3)
        self.c = nn.Linear(7, 3)        # never gets a gradient below


def _torch_adam_state(model, step_form):
    torch.manual_seed(0)
    ref = torch.optim.Adam(model.parameters(), lr=3e-3, betas=(0.5, 0.999))
    for _ in range(2):
        for n, p in model.named_parameters():
            p.grad = None if n.startswith("c.") else torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    if step_form == "int":              # torch 1.7 (what the reference pins) stores the step as a Python int
        for st in sd["state"].values():
            st["step"] = int(st["step"].item())
    return sd


@pytest.mark.parametrize("step_form", ["tensor", "int"])
def test_flat_adam_round_trips_a_torch_adam_state_dict(step_form):
    torch.manual_seed(1)
    model = _Tiny()
    sd = _torch_adam_state(model, step_form)
    opt = FlatAdam(_Tiny(), lr=1e-4, betas=(0.9, 0.999))
    opt.load_state_dict(sd)
    out = opt.state_dict()
    assert out["param_groups"][0]["betas"] == (0.5, 0.999) and out["param_groups"][0]["lr"] == 3e-3
    assert set(out["param_groups"][0]) == set(sd["param_groups"][0])
    assert set(out["state"]) == set(sd["state"]) == {0, 1, 2, 3}     # c.* never had a gradient: no state, as in torch
    for i, st in sd["state"].items():
        assert set(out["state"][i]) == set(st)
        assert torch.is_tensor(out["state"][i]["step"]) and float(out["state"][i]["step"]) == 2.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert out["state"][i][k].shape == st[k].shape and torch.equal(out["state"][i][k], st[k])
    # ... and back into a real torch.optim.Adam
    ref = torch.optim.Adam(_Tiny().parameters(), lr=1.0)
    ref.load_state_dict(out)
    back = ref.state_dict()
    assert set(back["param_groups"][0]) == set(out["param_groups"][0])
    for i, st in out["state"].items():
        assert torch.equal(back["state"][i]["exp_avg_sq"], st["exp_avg_sq"]) and float(back["state"][i]["step"]) == 2.0


def test_flat_adam_param_group_has_torch_adams_keys():
    ref = torch.optim.Adam(_Tiny().parameters(), lr=1e-3, betas=(0.5, 0.999))
    opt = FlatAdam(_Tiny(), lr=1e-3, betas=(0.5, 0.999))
    a, b = ref.state_dict()["param_groups"][0], opt.state_dict()["param_groups"][0]
    assert set(a) == set(b)
    assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    assert opt.state_dict()["state"] == {}


@pytest.mark.parametrize("key,val", [("amsgrad", True), ("maximize", True), ("nesterov", False)])
def test_flat_adam_refuses_what_it_cannot_honour(key, val):
    sd = _torch_adam_state(_Tiny(), "tensor")
    sd["param_groups"][0][key] = val
    with pytest.raises(ValueError, match=key):
        FlatAdam(_Tiny(), lr=1e-3).load_state_dict(sd)


def test_fused_adam_over_the_resnet_state_layout():
    """FusedAdam's state_dict indices / shapes are those of torch.optim.Adam(model.parameters()) over the same ResNet."""
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    from instaorder_amd import resnet_cls
    net = resnet_cls.resnet50_cls(in_channels=5, num_classes=2)
    opt = FusedAdam(net, lr=1e-3, betas=(0.5, 0.999))
    params = list(net.parameters())
    sd = {"state": {i: {"step": torch.tensor(3.0), "exp_avg": torch.full(p.shape, float(i)),
                        "exp_avg_sq": torch.full(p.shape, 2.0 * i)} for i, p in enumerate(params) if i % 7},
          "param_groups": [dict(torch.optim.Adam(params, lr=2e-3).state_dict()["param_groups"][0])]}
    opt.load_state_dict(sd)
    out = opt.state_dict()
    assert set(out["state"]) == set(sd["state"])
    for i, st in sd["state"].items():
        assert torch.equal(out["state"][i]["exp_avg"], st["exp_avg"]) and float(out["state"][i]["step"]) == 3.0
    assert opt.param_groups[0]["lr"] == 2e-3


class _Plan(_AdamFlat):
    def __init__(self, live, steps):
        self._params = [None] * len(live)
        self._live, self._steps = live, steps


def test_adam_launch_plan():
    """One launch when every parameter takes the update at one step count; a parameter that never had a gradient rides
    along only while weight decay is 0 (its update is then an exact no-op); otherwise runs split where the step count or
    liveness changes."""
    T, F = True, False
    assert _Plan([T] * 5, [2] * 5)._runs(0) == [(0, 4, 3)]
    assert _Plan([T, F, F, T, T], [1, 0, 0, 1, 1])._runs(0) == [(0, 4, 2)]
    assert _Plan([T, F, F, T, T], [1, 0, 0, 1, 1])._runs(1e-4) == [(0, 0, 2), (3, 4, 2)]
    assert _Plan([F, T, F, T], [0, 1, 0, 1])._runs(0) == [(0, 3, 2)]
    assert _Plan([T, F, T], [1, 1, 1])._runs(0) == [(0, 0, 2), (2, 2, 2)]      # had state: must stay untouched
    assert _Plan([T, T, T, T], [1, 1, 4, 4])._runs(0) == [(0, 1, 2), (2, 3, 5)]
    assert _Plan([F, F], [0, 0])._runs(0) == []


def _cfg(**kw):
    cfg = dict(algo="InstaOrderNet_o", lr=1e-3, weight_decay=1e-4, optim="Adam", beta1=0.5, backbone_arch="resnet50_cls",
               backbone_param=dict(in_channels=5, num_classes=2))
    cfg.update(kw)
    return cfg


def test_single_stage_model_adam_config():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    if torch.cuda.is_available():
        pytest.skip("constructs on the CPU")
    from instaorder_amd.single_stage_model import SingleStageModel
    m = SingleStageModel(_cfg())
    assert isinstance(m.optim, FusedAdam) and isinstance(m.optim, torch.optim.Optimizer)
    g = m.optim.param_groups[0]
    # the reference passes betas=(beta1, 0.999) and no weight decay (single_stage_model.py:39-42)
    assert g["betas"] == (0.5, 0.999) and g["weight_decay"] == 0 and g["lr"] == 1e-3 and g["eps"] == 1e-8
    cfg = _cfg()
    del cfg["beta1"]
    with pytest.raises(KeyError):
        SingleStageModel(cfg)
    with pytest.raises(Exception, match="No such optimizer: RMSprop"):
        SingleStageModel(_cfg(optim="RMSprop"))


def test_single_stage_model_adam_config_midas():
    if torch.cuda.is_available():
        pytest.skip("constructs on the CPU")
    from instaorder_amd.single_stage_model import SingleStageModel
    m = SingleStageModel(dict(algo="InstaDepthNet_d", lr=1e-4, weight_decay=1e-4, optim="Adam", beta1=0.9,
                              pretrained_weight=None))
    assert isinstance(m.optim, FlatAdam)
    g = m.optim.param_groups[0]
    assert g["betas"] == (0.9, 0.999) and g["weight_decay"] == 0
    assert len(m.optim._params) == len(list(m.net.parameters()))
    assert all(p.data_ptr() == m.optim.flat_params.data_ptr() + 4 * off
               for p, (off, _) in zip(m.optim._params, m.optim._spans))


def test_no_unprotected_16_byte_store_in_the_adam_kernel(tmp_path):
    """The Adam kernel's 16-byte stores under the store-hazard scan of tools/scan_store_hazard.py (see
    test_host_cpu.test_no_unprotected_16_byte_store_in_the_256_row_kernel)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    asm = str(tmp_path / "misc.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                           "-I" + os.path.join(ROOT, "instaorder_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-S",
                           "--cuda-device-only", os.path.join(ROOT, "instaorder_amd", "csrc", "misc.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    assert re.search(r"^_Z\w*adam_kernel\w*:", open(asm).read(), re.M), "adam_kernel is not in misc.hip's device code"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scan_store_hazard.py"), asm], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "hazard hits: 0" in p.stdout
