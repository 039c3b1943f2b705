#!/usr/bin/env python3
"""Every C-ABI call the wrappers of the 2-D convolution family make, as data: entry name, scalar arguments, WHICH tensor
stands at every pointer argument, and the profiler scope around the call.  No GPU and no library: `_call` is a recorder,
`_p` the identity (so the recorder sees tensors, not addresses), the size queries are fixed formulas of their arguments.

The drive goes through the three seams every layer passes -- conv2d._run_same (forward and input gradient, both kernels,
both arithmetics), conv2d._wgrad and gru.conv3x3_bf16 --, then the helper per kernel that tests reach by name, on small
CPU tensors.  tests/test_conv2d_call_trace_cpu.py replays it and compares with tests/golden/conv2d_call_trace.json
record by record: the library does the same work exactly when it is handed the same calls.

    python tools/make_conv2d_call_trace.py [out.json]      (default: tests/golden/conv2d_call_trace.json)
"""
import contextlib
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv2d_call_trace.json")
B, H, W = 2, 4, 5
# launch channels ci -> co, kh, kw, dilation, channels of the input rows (wider than ci: a channel slice of a wider tensor)
SAME = [(32, 32, 3, 3, 1, 32), (64, 32, 3, 3, 1, 64), (32, 64, 3, 3, 2, 32), (64, 64, 1, 1, 1, 64), (32, 32, 3, 5, 1, 32),
        (96, 32, 3, 3, 1, 96), (32, 32, 3, 3, 1, 64)]
# cm, cn, cm_real, cn_real, kh, kw, dilation, channels of the gradient rows, tag, late_ok
WGRAD = [(64, 32, 64, 32, 3, 3, 1, 64, "conv2d", True), (64, 64, 64, 64, 1, 1, 1, 96, "conv2d", True),
         (32, 32, 32, 32, 3, 5, 1, 32, "conv2d", True), (32, 32, 32, 27, 1, 1, 1, 32, "fe2d_first", False),
         (32, 64, 12, 40, 1, 1, 1, 32, "conv2d", True)]


class _Lib:
    """the size queries, as positive formulas that tell their arguments apart"""
    az_conv2d_packed_floats = staticmethod(lambda cin, cout, kh, kw: 3 * kh * kw * cin * cout + cin)
    az_conv2d_roll_packed_floats = staticmethod(lambda cin, cout: 27 * cin * cout + cout)
    az_conv2d_stats_tiles = staticmethod(lambda b, h, w, groups: (b // groups) * ((h + 7) // 8) * ((w + 15) // 16) + groups)
    az_conv2d_roll_stats_rows = staticmethod(
        lambda groups, b, h, w, cin, cout: 4 * (b // groups) * ((h + 7) // 8) * ((w + 15) // 16) + cin // 32 + 2 * (cout // 32))
    az_conv2d_wgrad_workspace = staticmethod(lambda cm, cn, kh, kw: 4 * (cm * cn * kh * kw + 2 * cm + cn))


class _Stats:  # (what the launchers need of a bn2d.Partials)
    def __init__(self, groups):
        self.groups, self.part, self.cnt, self.tiles = groups, None, None, None


class Recorder:
    def __init__(self, sigs):
        self.sigs, self.records, self.scopes, self.case, self.names, self.keep, self.given = sigs, [], [], None, {}, [], 0

    def begin(self, case, **tensors):
        """a new case; `tensors`: the caller's tensors by name (kept alive, so that no buffer allocated inside can take
        the address of one)"""
        self.case, self.names = case, {}
        self.keep = [t for t in tensors.values() if t is not None]
        self.given = len(self.keep)
        for name, t in tensors.items():
            if t is not None:
                assert t.data_ptr() not in self.names, (case, name)
                self.names[t.data_ptr()] = name

    def arg(self, a):
        if isinstance(a, torch.Tensor):
            if a.data_ptr() not in self.names:  # a buffer allocated inside: numbered in the order the calls show them
                self.names[a.data_ptr()] = f"new{len(self.keep) - self.given}:" + "x".join(map(str, a.shape))
                self.keep.append(a)
            return self.names[a.data_ptr()]
        assert a is None or isinstance(a, (int, float, str)), (self.case, type(a))
        return a

    def call(self, entry, *args):
        assert len(args) == len(self.sigs[entry]), (entry, len(args), "include/azhip.h declares", len(self.sigs[entry]))
        self.records.append({"case": self.case, "entry": entry, "args": [self.arg(a) for a in args],
                             "scope": self.scopes[-1] if self.scopes else None})

    @contextlib.contextmanager
    def scope(self, name, flops=0.0, bytes=0.0, bound="mfma", peak=None):
        self.scopes.append([name, flops, list(peak) if peak is not None else None])
        try:
            yield
        finally:
            self.scopes.pop()


@contextlib.contextmanager
def patched(rec):
    from activezero_amd import _lib, amax, conv2d, profiler
    from activezero_amd.nets.raft import gru
    todo = [(m, "_call", rec.call) for m in (conv2d, gru, amax)]
    todo += [(m, "_p", lambda t: t) for m in (conv2d, gru, amax)]
    todo += [(m, "_stream", lambda: "stream") for m in (conv2d, gru, amax)]
    todo += [(m, "_chk", lambda t, name, dtype=torch.float32: t) for m in (conv2d, gru)]
    todo += [(profiler, "scope", rec.scope), (_lib, "lib", lambda: _Lib)]
    saved = [(m, k, getattr(m, k)) for m, k, _ in todo]
    caches = [conv2d._PACK2D_CACHE, gru._PACK_CACHE, amax._W_AMAX]
    held = [dict(c) for c in caches]
    try:
        for m, k, v in todo:
            setattr(m, k, v)
        for c in caches:
            c.clear()
        yield conv2d, gru, amax
    finally:
        for m, k, v in saved:
            setattr(m, k, v)
        for c, h in zip(caches, held):
            c.clear()
            c.update(h)


def _t(*shape):
    return torch.zeros(*shape)


def trace():
    """the records of the whole drive"""
    from activezero_amd import _lib
    rec = Recorder(_lib._SIGS)
    with patched(rec) as (conv2d, gru, amax):
        for f16, flip, (ci, co, kh, kw, dil, cx), with_res in itertools.product((False, True), (False, True), SAME, (False, True)):
            for groups in (None, 1, 2):
                if groups is not None and (with_res or flip or (kh, kw) not in ((3, 3), (1, 1))):
                    continue  # (the statistics launch: a layer's forward without epilogue operands, 3x3 and 1x1)
                x, res = _t(B, H, W, cx), _t(B, H, W, co) if with_res else None
                weight = _t(ci, co, kh, kw) if flip else _t(co, ci, kh, kw)
                x_amax = _t(amax.AMAX_SLOTS) if (f16 and flip) else None  # the gradient's producer attached one
                rec.begin(f"run_same f16={int(f16)} flip={int(flip)} {ci}->{co} {kh}x{kw}d{dil} cx={cx} res={int(with_res)} "
                          f"stats={groups}", x=x, weight=weight, res=res, x_amax=x_amax)
                if x_amax is not None:
                    amax._set_amax(x, x_amax)
                stats = _Stats(groups) if groups is not None else None
                out = conv2d._run_same(x, x, weight, ci, co, kh, kw, dil, flip, f16, res=res,
                                       tag="dgrad2d" if flip else "conv2d", stats=stats)
                rec.records.append({"case": rec.case, "result": list(out.shape), "stats": None if stats is None else
                                    [list(stats.part.shape), list(stats.cnt.shape), stats.tiles]})
        for (cm, cn, cm_real, cn_real, kh, kw, dil, cg, tag, late_ok), how in itertools.product(WGRAD, ("x6", "f16", "f16+amax")):
            gr, xr = _t(B, H, W, cg), _t(B, H, W, cn)
            am = (_t(amax.AMAX_SLOTS), _t(amax.AMAX_SLOTS)) if how == "f16+amax" else (None, None)
            rec.begin(f"wgrad {how} {cm}({cm_real})x{cn}({cn_real}) {kh}x{kw}d{dil} cg={cg} {tag}", gr=gr, xr=xr, am_g=am[0], am_x=am[1])
            gw = conv2d._wgrad(gr, xr, cm, cn, cm_real, cn_real, kh, kw, dil, tag=tag, sink=None,
                               amax=None if how == "x6" else am, late_ok=late_ok)
            rec.records.append({"case": rec.case, "result": list(gw.shape)})
        # the helper per kernel of before the table, by name: every pack helper fresh and memoised, every run helper with the
        # operands its callers pass
        for cache in (False, True):
            w = _t(12, 40, 1, 1)
            rec.begin(f"_pack cache={int(cache)}", weight=w)
            pk = conv2d._pack(w, 48, 32, 40, 12, 40, 1, 1, 1, False, cache=cache)
            rec.records.append({"case": rec.case, "result": rec.arg(pk)})
            w = _t(12, 40, 1, 1)
            rec.begin(f"_pack_f16 cache={int(cache)}", weight=w)
            pk, am = conv2d._pack_f16(w, 48, 32, 40, 12, 40, 1, 1, 1, True, cache=cache)
            rec.records.append({"case": rec.case, "result": [rec.arg(pk), rec.arg(am)]})
            w = _t(32, 64, 3, 3)
            rec.begin(f"_pack_roll cache={int(cache)}", weight=w)
            pk = conv2d._pack_roll(w, 64, 32, 64 * 9, 9, False, cache=cache)
            rec.records.append({"case": rec.case, "result": rec.arg(pk)})
        w = _t(32, 64, 3, 3)
        rec.begin("_pack_roll_f16", weight=w)
        pk, am = conv2d._pack_roll_f16(w, 32, 64, 9, 32 * 9, True)
        rec.records.append({"case": rec.case, "result": [rec.arg(pk), rec.arg(am)]})
        x, pk, sc, sh, res = _t(B, H, W, 32), _t(100), _t(64), _t(64), _t(B, H, W, 96)
        xa, wa = _t(amax.AMAX_SLOTS), _t(amax.AMAX_SLOTS)
        rec.begin("_run helpers", x=x, packed=pk, scale=sc, shift=sh, res=res, x_amax=xa, w_amax=wa)
        conv2d._run(x, pk, 32, 64, 3, 3, 2, sc, sh, res, True, tag="conv2d_eval")
        conv2d._run(x, pk, 32, 64, 1, 1, 1, stats=_Stats(2))
        conv2d._run_f16(x, xa, pk, wa, 32, 64, 3, 3, 1, scale=sc, shift=sh, res=res, relu=True)
        conv2d._run_f16(x, xa, pk, wa, 32, 64, 3, 3, 1, stats=_Stats(1))
        conv2d._run_roll(x, pk, 32, 64, scale=sc, shift=sh, res=res, relu=True)
        conv2d._run_roll(x, pk, 32, 64, stats=_Stats(2))
        conv2d._run_roll_f16(x, xa, pk, wa, 32, 64, res=res, tag="dgrad2d")
        conv2d._run_roll_f16(x, xa, pk, wa, 32, 64, stats=_Stats(1))
        cin, cout = 32, 64
        for h1, cx, operands in itertools.product((False, True), (32, 48), ("", "bias", "bias res", "bias res gates", "amax", "bias res amax")):
            xr, packed = _t(B, H, W, cx), _t(9 * cin * cout // 2)
            bias = _t(cout) if "bias" in operands else None
            res = _t(B, H, W, cout + 32) if "res" in operands else None
            gz, gh = (_t(B, H, W, 2 * cout), _t(B, H, W, cout)) if "gates" in operands else (None, None)
            am = _t(amax.AMAX_SLOTS) if "amax" in operands else None
            act = gru.ACT_GRU if gz is not None else (gru.ACT_SIGMOID if res is not None else gru.ACT_NONE)
            rec.begin(f"gru conv3x3 h1={int(h1)} cx={cx} [{operands}]", xr=xr, packed=packed, bias=bias, residual=res, gate_z=gz,
                      gate_h=gh, in_amax=am)
            out = gru.conv3x3_bf16(xr, packed, cin, cout, bias, res, act, gz, gh, h1=h1, in_amax=am)
            rec.records.append({"case": rec.case, "result": list(out.shape)})
    return json.loads(json.dumps(rec.records))  # (as the golden file holds them: tuples are lists)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    records = trace()
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
    print(f"{len(records)} records -> {out}")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
