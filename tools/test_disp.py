#!/usr/bin/env python3
"""Dense-disparity evaluation of a MiDaS net: tools/test_disp_KITTI.py and tools/test_disp_DIW.py of the reference in one
command, batched on the GPU (instaorder_amd.dense_eval).

    python tools/test_disp.py --config experiments/kitti/InstaDepthNet_d/config.yaml --load_model ckpt.pth.tar
    python tools/test_disp.py --config experiments/DIW/midas_pretrained/config.yaml --load_model model-f6b98070.pt

The YAML is the reference's: ``data.dataset`` is 'kitti' or 'diw', ``model.algo`` is 'midas_pretrained' (a bare
MidasNet loaded from --load_model) or 'InstaDepthNet_d' / 'InstaDepthNet_od' (the wrapper, then load_state and eval).
``--test_num`` N > 0 evaluates the first N images (-1: all).  Added: ``--batch`` and ``--dtype fp32|bf16``.  Prints the
reference's result lines.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", required=True, type=str)
    p.add_argument("--load_model", required=True, type=str)
    p.add_argument("--test_num", default=-1, type=int)
    p.add_argument("--batch", default=0, type=int, help="images per forward (default: 4 for kitti, 8 for diw)")
    p.add_argument("--dtype", default="fp32", choices=("fp32", "bf16"))
    return p.parse_args(argv)


def load_config(path):
    """The reference's YAML with its path rewriting: test_disp_KITTI.py prefixes '/data/' strings with '' (BASE_DIR),
    test_disp_DIW.py with data.base_dir."""
    import yaml
    with open(path) as f:
        config = yaml.safe_load(f)
    base = config["data"].get("base_dir", "") if config["data"].get("dataset") == "diw" else ""
    for v in config.values():
        if isinstance(v, dict):
            for k, s in v.items():
                if isinstance(s, str) and "/data/" in s:
                    v[k] = "%s%s" % (base, s)
    return config


def build_model(model_cfg, load_model, dtype):
    import torch
    algo = model_cfg["algo"]
    if algo == "midas_pretrained":
        from instaorder_amd.midas_net import MidasNet
        model = MidasNet(load_model, non_negative=True)
        model.dtype = dtype
        model.cuda()
        model.eval()
        return model
    if algo not in ("InstaDepthNet_d", "InstaDepthNet_od"):
        raise Exception("No such algo for dense evaluation: {}".format(algo))
    import instaorder_amd as ia
    cfg = dict(model_cfg, dtype=dtype)
    model = getattr(ia, algo)(cfg, dist_model=False)
    model.load_state(load_model)
    model.switch_to("eval")
    torch.cuda.synchronize()
    return model


def main(argv=None):
    args = parse_args(argv)
    config = load_config(args.config)
    from instaorder_amd import dense_eval
    data, model_cfg = config["data"], config["model"]
    algo = model_cfg["algo"]
    model = build_model(model_cfg, args.load_model, args.dtype)
    mean, std = data.get("data_mean", (0.485, 0.456, 0.406)), data.get("data_std", (0.229, 0.224, 0.225))
    if data["dataset"] == "kitti":
        reader = dense_eval.KITTIEigenReader(data["val_annot_file"], data["val_image_root"], args.test_num)
        r = dense_eval.eval_dense_depth(model, reader, algo, batch=args.batch or 4, min_depth=1e-3, max_depth=80,
                                        data_mean=mean, data_std=std)
        print("computed error on {} / {} missing".format(r["n_images"], r["missing"]))
        print("\n  " + ("{:>8} | " * 8).format("abs_rel", "sq_rel", "rmse", "rmse_log", "d1", "d2", "d3", "silog"))
        print(("{: 8.3f}  " * 8).format(*[r[k] for k in dense_eval.ERROR_NAMES]) + "\\\\")
        print("\n-> Done!")
    elif data["dataset"] == "diw":
        reader = dense_eval.DIWReader(data["val_annot_file"], data["val_image_root"], args.test_num)
        r = dense_eval.eval_ordinal_via_disp(model, reader, algo, batch=args.batch or 8, data_mean=mean, data_std=std)
        print("computed error on {}".format(r["total"]))
        print("wrong/all = {}/{}".format(r["wrong"], r["total"]))
        print("WHDR = {}".format(r["WHDR"]))
    else:
        raise NotImplementedError("dataset '%s' (kitti | diw)" % data["dataset"])
    return r


if __name__ == "__main__":
    main()
