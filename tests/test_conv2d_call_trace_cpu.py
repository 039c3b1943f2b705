"""The wrappers of the 2-D convolution family (activezero_amd/conv2d.py, nets/raft/gru.py) hand the library the calls
tests/golden/conv2d_call_trace.json holds: per C-ABI call the entry name, every scalar, which tensor stands at every
pointer argument (the caller's by name, a buffer allocated inside by order and shape) and the profiler scope around it,
over conv2d._run_same (both kernels, both arithmetics, forward and flipped, residual, BatchNorm partials),
conv2d._wgrad, gru.conv3x3_bf16 and the helper per kernel (conv2d._pack* / _run*).  The golden file was recorded by tools/make_conv2d_call_trace.py before the
wrappers became one kernel table, one packer and one launcher; the library is handed the same calls, so it does the
same work.

Pure host logic: recorders instead of the library, CPU tensors as stand-ins."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_conv2d_call_trace", os.path.join(ROOT, "tools", "make_conv2d_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_abi_call_is_the_recorded_one():
    tool = _tool()
    with open(tool.GOLDEN) as f:
        want = json.load(f)
    got = tool.trace()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), (len(got), len(want))
    # (the drive reached every entry of the family's launch and pack surface)
    entries = {r["entry"] for r in want if "entry" in r}
    assert entries >= {"az_conv2d_fwd", "az_conv2d_fwd_stats", "az_conv2d_fwd_f16", "az_conv2d_fwd_stats_f16", "az_conv2d_roll_fwd",
                       "az_conv2d_roll_fwd_stats", "az_conv2d_roll_fwd_f16", "az_conv2d_roll_fwd_stats_f16", "az_conv2d_bf16_fwd",
                       "az_conv2d_h1_fwd", "az_conv2d_pack_weights", "az_conv2d_pack_weights_f16", "az_conv2d_roll_pack",
                       "az_conv2d_roll_pack_f16", "az_conv2d_wgrad", "az_conv2d_wgrad_f16"}, sorted(entries)


def test_the_recorders_are_taken_out_again():
    from activezero_amd import _lib, conv2d, ops, profiler
    tool = _tool()
    before = (_lib.lib, conv2d._call, conv2d._p, profiler.scope)
    tool.trace()
    assert (_lib.lib, conv2d._call, conv2d._p, profiler.scope) == before and conv2d._call is ops._call
