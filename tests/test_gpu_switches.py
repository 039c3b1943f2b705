"""Every route that only an A/B switch reaches (DESIGN.md, table "A/B switches") is run through existing parity tests in a
child process with the switch set: a route that ships is a route that is tested.  The switches are read once per
process (az_options.h / module import), hence the child processes -- one at a time."""
import os
import subprocess
import sys

import pytest

from tests.test_options_cpu import RETIRED

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    # (environment, test file, -k expression)
    ({"AZ_CONV_ROLL": "0"}, "tests/test_gpu_conv3d.py", "convbn3d_golden and bf16x6"),                # V0 layers on az_conv3d_m128.hip
    ({"AZ_WGRAD_R16": "0"}, "tests/test_gpu_conv3d.py", "residual_relu_train and bf16x6"),             # one-kd-per-wave stride-1 weight gradient
    ({"AZ_WGRAD_R16": "0", "AZ_WGRAD_ORDER": "0"}, "tests/test_gpu_conv3d.py", "residual_relu_train and bf16x6"),  # its work list in linear order
    ({"AZ_WGRAD_R16": "0", "AZ_WGRAD_SLOTS": "512"}, "tests/test_gpu_conv3d.py", "residual_relu_train and bf16x6"),  # a quarter of the resident waves
    ({"AZ_WGRAD_R16": "1"}, "tests/test_gpu_conv3d.py", "convbn3d_golden and bf16x6"),
    ({"AZ_BWD_F16": "0"}, "tests/test_gpu_conv3d.py", "convbn3d_golden and bf16x6"),                   # bf16x6 gradients
    ({"AZ_CONV_MAP": "0"}, "tests/test_gpu_conv3d.py", "conv_stride2_vs_torch"),                       # linear block -> tile map
    ({"AZ_CONV2D_ROLL": "0"}, "tests/test_gpu_conv2d.py", "same"),                                     # 32/64-channel 3x3 layers on K13
    ({"AZ_CONV2D_WGRAD_R16": "0"}, "tests/test_gpu_conv2d.py", "same"),
    ({"AZ_PATCH_TILED": "0"}, "tests/test_gpu_kernels.py", "patch"),
    ({"AZ_WGRAD_R16_WGS": "64", "AZ_ROLL_SEGLEN": "5"}, "tests/test_gpu_conv3d.py", "convbn3d_golden"),
    ({"AZ_WGRAD_S2R16": "0"}, "tests/test_gpu_conv3d.py", "weight_grad_stride2 and f16x3"),            # stride-2 f16x3 weight gradient, one kd per wave
    ({"AZ_WGRAD_R16_XCD": "0"}, "tests/test_gpu_conv3d.py", "residual_relu_train and f16x3"),           # K4w columns in linear order
    ({"AZ_CONV_T2ROLL": "0"}, "tests/test_gpu_conv3d.py", "(deconv or hourglass_golden) and f16x3"),       # transposed 64 -> 32 on az_conv3d_t2.hip
    ({"AZ_CONV_S2ROLL": "0"}, "tests/test_gpu_conv3d.py", "(conv_stride2 or hourglass_golden or presplit_routing) and f16x3 or presplit_routing"),  # stride-2 32 -> 64 on the gather kernel
    ({"AZ_S2ROLL_SEGLEN": "1"}, "tests/test_gpu_s2roll.py", "forward or partials or input_gradient"),
    ({"AZ_CONV_ROLL64": "0"}, "tests/test_gpu_conv3d.py", "(conv_stride1 or convbn3d_golden or hourglass_golden) and f16x3"),        # stride-1 64 -> 64 on the gather kernel                               # one output plane per depth segment
    ({"AZ_GRU_ASSEMBLE": "0"}, "tests/test_gpu_raft_gru.py", "golden or fused_training_node"),      # the GRU's input rows by torch slice assignments
    ({"AZ_LOOKUP_ACC": "0"}, "tests/test_gpu_raft_corr.py", "golden or vs_torch_ops"),                # one gradient buffer per lookup and level
    # the Python-level switches of the two-stream backward (overlap.py, conv2d.py)
    ({"AZ_SIDE_RELEASE": "record"}, "tests/test_gpu_overlap.py", "in_order_pass or partial_backward or two_forward"),  # operands released through record_stream
    ({"AZ_SIDE_PRIORITY": "-1"}, "tests/test_gpu_overlap.py", "in_order_pass"),             # side stream at the other HIP priority
    ({"AZ_2D_WGRAD_OVERLAP": "0"}, "tests/test_gpu_overlap.py", "in_order_pass"),           # 2-D weight gradients in order
    ({"AZ_PRESPLIT": "0"}, "tests/test_gpu_conv3d.py", "(convbn3d_golden or residual_relu_train or hourglass_golden) and f16x3"),  # fp32 gradient operands, split by the consumers
    ({"AZ_PACK_PLAN": "0"}, "tests/test_gpu_psmnet.py", "train and not d192 and not full_size"),           # every weight image packed by its own launch
    ({"AZ_GRAD_HANDOVER": "0"}, "tests/test_gpu_conv3d.py", "hourglass_golden or handover"),             # every consumer returns its own gradient, the engine adds
    ({"AZ_WGRAD_DEFER": "0"}, "tests/test_gpu_overlap.py", "in_order_pass or partial_backward"),            # per-layer workspace memset + unpack on the side stream
    ({"AZ_DEBUG_AMAX": "1"}, "tests/test_gpu_conv3d.py", "(convbn3d_golden or residual_relu_train) and f16x3"),  # every attached amax checked against a fresh pass
]


# The stride-1 sweep against fp64 (tests/test_gpu_conv3d_s1.py) behind every switch that changes one of its routes; each
# selection also runs that file's route-coverage test under the switch.
S1 = "tests/test_gpu_conv3d_s1.py"
S1_WGRAD = "stride1_vs_fp64 and wgrad and not fp32 or presplit_operands or accumulate_only or every_route"
# the bf16x6 forward launches off the rolling kernel, their epilogues (partials; affine + residual + ReLU) element-wise too
S1_GATHER_X6 = ("(stride1_vs_fp64 or residual_handover) and bf16x6 and not wgrad or every_route"
                " or (forward_batchnorm_partials or forward_affine_residual_relu_epilogue) and bf16x6")
# the block -> tile maps (az_conv_tile_decode) at the shapes with more than one tile row, column, plane or batch entry
S1_TILE_MAP = "stride1_vs_fp64 and fwd and bf16x6 and (2x4x9x16 or 3x2x5x33 or 1x13x25x17) or every_route"
S1_CASES = [
    ({"AZ_WGRAD_R16_WGS": "3"}, S1, S1_WGRAD),                   # the column walk at every shape with more than 3 columns
    ({"AZ_WGRAD_R16_WGS": "8"}, S1, S1_WGRAD),                   # wgs % 8 == 0: the XCD column map at small shapes
    ({"AZ_WGRAD_R16_WGS": "64"}, S1, "stride1_vs_fp64 and wgrad and 1x24x5x352 or every_route"),  # the cap takes effect
    ({"AZ_WGRAD_R16_XCD": "0"}, S1, S1_WGRAD + " or full_size"),
    ({"AZ_WGRAD_R16": "0"}, S1, "stride1_vs_fp64 and wgrad and bf16x6 or every_route"),  # one-kd-per-wave bf16x6 kernels
    ({"AZ_WGRAD_R16": "1"}, S1, "stride1_vs_fp64 and wgrad and bf16x6 or every_route"),
    ({"AZ_CONV_ROLL": "0"}, S1, S1_GATHER_X6),                     # m128: a dead lower half patch at 1x13x25x17
    ({"AZ_CONV_ROLL": "0", "AZ_CONV_M128": "0"}, S1, S1_GATHER_X6),  # the gather kernel: a ragged band at 1x13x25x17
    ({"AZ_CONV_ROLL64": "0"}, S1, "(stride1_vs_fp64 or residual_handover) and f16x3 and 64x64 and not wgrad or every_route"),
    ({"AZ_ROLL_SEGLEN": "1"}, S1, "stride1_vs_fp64 and not wgrad and not fp32 or residual_handover or dgrad_presplit or full_size"),
    # multi-plane segments at small shapes (depth 13: 5, 5 and 3 planes; depth 5: one of five): the partials' carried state
    ({"AZ_ROLL_SEGLEN": "5"}, S1, "forward_batchnorm_partials or forward_affine_residual_relu_epilogue or every_route"),
    ({"AZ_CONV_ROLL": "0", "AZ_CONV_MAP": "0"}, S1, S1_TILE_MAP),   # m128 and the gather kernel on the linear block -> tile map
    ({"AZ_CONV_ROLL": "0", "AZ_CONV_MAP": "1"}, S1, S1_TILE_MAP),   # ... on the XCD chunks without bands
]


# The 2-D sweep against fp64 (tests/test_gpu_conv2d_fp64.py) behind the two switches that change its routes; each selection
# also runs that file's route-coverage test under the switch.
C2D = "tests/test_gpu_conv2d_fp64.py"
C2D_CASES = [
    ({"AZ_CONV2D_ROLL": "0"}, C2D, "conv_vs_fp64 and (32x or 64x) or residual_handover or every_route"),  # the roll layers on K13
    ({"AZ_CONV2D_WGRAD_R16": "0"}, C2D, "wgrad_vs_fp64 and (32x or 64x) or accumulate_only or every_route"),  # ... on K13w
]


# The strided sweep against fp64 (tests/test_gpu_conv3d_s2.py) behind every switch that changes one of its routes; each
# selection also runs that file's route-coverage test under the switch (which asserts, for the AZ_S2ROLL_SEGLEN rows, that
# multi-plane and ragged segments are among the cases).
S2 = "tests/test_gpu_conv3d_s2.py"
S2_MODE1_3264 = "f16x3 and (s2-fwd-32x64 or t2-dgrad-64x32) or every_route"   # the launches of mode 1, 32 -> 64
S2_MODE2_6432 = "f16x3 and (t2-fwd-64x32 or s2-dgrad-32x64) or every_route"   # the launches of mode 2, 64 -> 32
S2_MULTI_TILE = "2x6x8x20 or 3x4x18x30 or 1x14x50x34 or 2x3x4x17 or 3x2x9x15 or 1x7x25x17"
S2_CASES = [
    ({"AZ_CONV_S2ROLL": "0"}, S2, S2_MODE1_3264),                 # ... on the gather kernel
    ({"AZ_CONV_T2ROLL": "0"}, S2, S2_MODE2_6432),                 # ... on az_conv3d_t2.hip
    ({"AZ_WGRAD_S2R16": "0"}, S2, "wgrad and f16x3 or accumulate_only or every_route"),  # f16x3 weight gradients, one kd per wave
    ({"AZ_S2ROLL_SEGLEN": "3"}, S2, S2_MODE1_3264),               # multi-plane segments, ragged where Do % 3
    ({"AZ_S2ROLL_SEGLEN": "2"}, S2, S2_MODE1_3264),
    ({"AZ_CONV_MAP": "0"}, S2, f"strided_vs_fp64 and not wgrad and ({S2_MULTI_TILE}) or every_route"),  # linear block -> tile map
    ({"AZ_CONV_MAP": "1"}, S2, f"strided_vs_fp64 and not wgrad and ({S2_MULTI_TILE}) or every_route"),  # XCD chunks without bands
    ({"AZ_PRESPLIT": "0"}, S2, "presplit or accumulate_only or every_route"),  # the pre-split tests skip, the rest pass
]


# The reprojection sweep against fp64 (tests/test_gpu_reproj_fp64.py) with K8 on the per-pixel kernel: every K8 test (the
# million-pixel case among them: tiled by default, the per-pixel kernel's grid-stride loop here) and that file's route-coverage
# test, which asserts under the switch that every K8 case is per-pixel.
REPROJ = "tests/test_gpu_reproj_fp64.py"
REPROJ_CASES = [
    ({"AZ_PATCH_TILED": "0"}, REPROJ, "k8 or every_route or largest_ratios"),
]


# The non-finite sweep (tests/test_gpu_nonfinite.py) on the one forward route that only a switch reaches: the bf16x6 32-channel
# stride-1 layers on az_conv3d_m128.hip; that file's route-coverage test asserts under the switch that they are there.
NONFINITE = "tests/test_gpu_nonfinite.py"
NONFINITE_CASES = [
    ({"AZ_CONV_ROLL": "0"}, NONFINITE, "conv3d_s1 and bf16x6 or every_forward_route or rolling_kernels"),
]


def _child(env, path, expr):
    cmd = [sys.executable, "-m", "pytest", path, "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    if expr:
        cmd += ["-k", expr]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, tail


@pytest.mark.parametrize("env,path,expr", CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in CASES])
def test_route_behind_switch(env, path, expr):
    _child(env, path, expr)


@pytest.mark.parametrize("env,path,expr", S1_CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in S1_CASES])
def test_stride1_sweep_behind_switch(env, path, expr):
    _child(env, path, expr)


@pytest.mark.parametrize("env,path,expr", C2D_CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in C2D_CASES])
def test_conv2d_sweep_behind_switch(env, path, expr):
    _child(env, path, expr)


@pytest.mark.parametrize("env,path,expr", S2_CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in S2_CASES])
def test_strided_sweep_behind_switch(env, path, expr):
    _child(env, path, expr)


@pytest.mark.parametrize("env,path,expr", REPROJ_CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in REPROJ_CASES])
def test_reprojection_sweep_behind_switch(env, path, expr):
    _child(env, path, expr)


@pytest.mark.parametrize("env,path,expr", NONFINITE_CASES, ids=[" ".join(f"{k}={v}" for k, v in c[0].items()) for c in NONFINITE_CASES])
def test_nonfinite_sweep_behind_switch(env, path, expr):
    _child(env, path, expr)


def test_switches_are_read_once_into_the_options_struct():
    """az_option reports what the library holds; changing the environment afterwards changes nothing"""
    code = ("import os; os.environ['AZ_WGRAD_R16_WGS']='77'; from activezero_amd import _lib; L=_lib.lib(); "
            "a=L.az_option(b'AZ_WGRAD_R16_WGS'); os.environ['AZ_WGRAD_R16_WGS']='5'; b=L.az_option(b'AZ_WGRAD_R16_WGS'); "
            "print(a, b, L.az_option(b'AZ_WGRAD_R16'), L.az_option(b'NOPE'), L.az_option(b'%s'))" % RETIRED[0])
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    a, b, k, nope, retired = r.stdout.split()
    assert (a, b, k) == ("77", "77", "2") and int(nope) < 0
    assert int(retired) < 0  # a switch that was taken out is no switch
