#!/usr/bin/env python3
"""Launch trace of one ResNet-50 training step (io_net_forward + io_net_backward, and the backward again as one
io_net_backward_stages call per stage): per case the launch list [(class, flops, bytes)] in execution order, and the
SHA-256 of the logits and of the flat gradient where two runs of the same library give the same bits.

The record of a commit is what a refactor of the executor (csrc/net.hip) is held to: tests/test_gpu_step_routes.py reruns
CASES and asserts the lists and hashes of tests/golden/step_launch_trace.json.  Uses engine.prof_begin / prof_launches only.
Also records the workspace layout (io_net_workspace_bytes, io_net_activation_offset) of tests/test_step_routes_cpu.py.
usage: python tools/step_trace.py [--layout-only] OUT.json      (on the commit to record; rewrites the "cases" / "cu_count"
       keys -- on an MI355X -- and the "layout" key -- anywhere -- of OUT.json)"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

# (dtype, N, S, G, io_set_bf16_p256 mode, io_set_bf16_p256_xop); fp32 takes neither switch (set to the defaults)
CASES = [("fp32", 4, 64, 1, 1, 1), ("fp32", 3, 96, 1, 1, 1), ("fp32", 16, 128, 2, 1, 1),
         ("bf16", 16, 128, 1, 3, 1), ("bf16", 16, 128, 1, 3, 0), ("bf16", 16, 128, 1, 1, 1),
         ("bf16", 16, 128, 2, 3, 1)]


def case_id(case):
    return "%s-n%d-s%d-g%d-p256_%d-xop%d" % case


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(case):
    """-> dict(whole=[[class, flops, bytes]], staged=[...], logits=sha, grads=sha, grads_staged=sha)"""
    from instaorder_amd import _lib, engine, resnet_cls
    dtype, N, S, G, mode, xop = case
    lib = _lib.lib()
    prev = lib.io_set_bf16_p256(mode), lib.io_set_bf16_p256_xop(xop)
    try:
        torch.manual_seed(1234 + N + S)
        net = resnet_cls.ResNet(5, [2, 3], dtype=dtype).cuda()
        net.train()
        gen = torch.Generator().manual_seed(77 + N * S)
        x8 = engine.pack_nchw(torch.randn(N, 5, S, S, generator=gen).cuda(), dtype=dtype)
        dl = (torch.randn(N, net.plan.num_logits, generator=gen) * 0.01).cuda()
        out = {}

        def traced(fn):
            torch.cuda.synchronize()
            engine.prof_begin()
            try:
                r = fn()
                torch.cuda.synchronize()
                recs = engine.prof_launches()
            finally:
                engine.prof_end()
            return r, [[name, fl, by] for name, _ms, fl, by in recs]

        def whole():
            logits, ws = net._run_forward(x8, N, S, G, True)
            net._run_backward(x8, dl, N, S, G, ws)
            return logits, ws
        (logits, ws), out["whole"] = traced(whole)
        out["logits"], out["grads"] = _sha(logits), _sha(net.flat_grads)
        net._pool.give(ws)
        net.flat_grads.zero_()

        def staged():
            logits, ws = net._run_forward(x8, N, S, G, True)
            for s in range(net.plan.backward_stages):
                net._run_backward(x8, dl, N, S, G, ws, stages=(s, s + 1))
            return logits, ws
        (logits, ws), out["staged"] = traced(staged)
        out["grads_staged"] = _sha(net.flat_grads)
        net._pool.give(ws)
        return out
    finally:
        lib.io_set_bf16_p256(prev[0])
        lib.io_set_bf16_p256_xop(prev[1])


def cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


LAYOUT_SHAPES = ((4, 64), (3, 96), (16, 128), (32, 256), (256, 256))


def layout():
    """{"dtype-nN-sS": [training bytes, eval bytes, offset of which = 0, 2, 3 .. 18]}: io_net_workspace_bytes and
    io_net_activation_offset (host arithmetic: no GPU)"""
    from instaorder_amd import engine
    out = {}
    for dtype in ("fp32", "bf16"):
        net = engine.Net(5, [2, 3], dtype)
        for N, S in LAYOUT_SHAPES:
            out["%s-n%d-s%d" % (dtype, N, S)] = [net.workspace_bytes(N, S, True), net.workspace_bytes(N, S, False)] + \
                [net.activation_offset(N, S, w) for w in [0] + list(range(2, 19))]
    return out


def main(path, layout_only=False):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["layout"] = layout()
    if not layout_only:
        trace(doc)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


def trace(doc):
    doc["cu_count"] = cu_count()
    doc["cases"] = {}
    for case in CASES:
        a, b = run_case(case), run_case(case)
        assert a["whole"] == b["whole"] and a["staged"] == b["staged"], case_id(case)
        rec = dict(whole=a["whole"], staged=a["staged"])
        for k in ("logits", "grads", "grads_staged"):      # a hash only where this library repeats its own bits
            if a[k] == b[k]:
                rec[k] = a[k]
        doc["cases"][case_id(case)] = rec
        print("%s: %d + %d launches, stable: %s" % (case_id(case), len(rec["whole"]), len(rec["staged"]),
                                                    [k for k in ("logits", "grads", "grads_staged") if k in rec]))


if __name__ == "__main__":
    main(sys.argv[-1], layout_only="--layout-only" in sys.argv[1:-1])
