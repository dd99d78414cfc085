"""The operator layer (instaorder_amd/ops.py) keeps ONE copy of each launch block: every convolution / BatchNorm entry
point of the library is launched from exactly one place in the file, and the autograd nodes compose those helpers.  A
fused path that pastes a block back in fails here."""
import os
import re

import pytest

from helpers import ROOT

ONE_CALL_SITE = ["io_conv2d_fwd_dt", "io_conv2d_fwd_bias_dt", "io_conv2d_fwd_bnstats_dt", "io_conv2d_dgrad_dt",
                 "io_conv2d_dgrad_bnbwd_dt", "io_conv2d_wgrad_dt", "io_conv2d_wgrad_workspace_bytes", "io_gconv_pack",
                 "io_gconv2d_fwd", "io_gconv2d_dgrad", "io_gconv2d_wgrad", "io_gconv_unpack_grad", "io_bn_stats_finalize_dt",
                 "io_bn_eval_prepare", "io_bn_apply_dt", "io_bn_bwd_dt", "io_bn_partial_floats", "io_add"]


@pytest.mark.parametrize("name", ONE_CALL_SITE)
def test_entry_point_has_one_call_site_in_ops(name):
    with open(os.path.join(ROOT, "instaorder_amd", "ops.py")) as f:
        src = f.read()
    sites = re.findall(r"\b(?:L|_L\(\))\.%s\(" % re.escape(name), src)
    assert len(sites) == 1, (name, len(sites))
