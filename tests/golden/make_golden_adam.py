#!/usr/bin/env python3
"""Golden vectors for ``optim: Adam``: the REAL reference's InstaOrderNet_o / InstaOrderNet_od built with
``optim: Adam`` and beta1 = 0.5 (models/single_stage_model.py:39-42: torch.optim.Adam(lr, betas=(beta1, 0.999)), no
weight decay), three training steps on the CPU exactly as make_golden.case_train records them (same shims, same helpers,
imported from make_golden.py).  Extra keys: ``beta1`` and ``optim``.

Runs only where the reference checkout exists (never on the GPU box); no test reads the reference.
usage: python tests/golden/make_golden_adam.py [adam_o_S64_B4] [adam_od_S64_B4]"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402

BETA1 = 0.5
_model_cfg = mg.model_cfg


def adam_model_cfg(algo):
    cfg = dict(_model_cfg(algo))
    cfg["optim"], cfg["beta1"] = "Adam", BETA1
    return cfg


def case_train_adam(algo, S, B, seed, steps, tag):
    mg.model_cfg = adam_model_cfg          # what make_golden.build() reads the model section through
    try:
        mg.case_train(algo, S, B, seed, steps, tag)
    finally:
        mg.model_cfg = _model_cfg
    path = os.path.join(mg.HERE, tag + ".npz")
    out = dict(np.load(path, allow_pickle=False))
    out["beta1"] = np.float64(BETA1)
    out["optim"] = np.array("Adam")
    np.savez_compressed(path, **out)


CASES = {
    "adam_o_S64_B4": lambda: case_train_adam("InstaOrderNet_o", 64, 4, 41, 3, "adam_o_S64_B4"),
    "adam_od_S64_B4": lambda: case_train_adam("InstaOrderNet_od", 64, 4, 42, 3, "adam_od_S64_B4"),
}

if __name__ == "__main__":
    which = sys.argv[1:] or list(CASES)
    mg.install_shims()
    mg.init_dist(0, 1, 29533)
    torch.manual_seed(0)
    for c in which:
        CASES[c]()
