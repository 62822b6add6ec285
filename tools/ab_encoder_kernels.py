#!/usr/bin/env python
"""Two builds of libsrbh against each other on the depthwise conv and the encoder's inference kernels (csrc/srbh_dwconv.hip,
csrc/srbh_enc_eval.hip): same bits, same speed.

    python tools/ab_encoder_kernels.py --parent-lib /path/to/parent/libsrbh.so [--tree-lib ...] [--rounds 9] [--only bits|bench] [--no-bench-py]

Both libraries (one ABI) are loaded into ONE process; the Python layer of this tree drives either (tools/ab_raster_walk.py's method).
  bits   sha256 of every output buffer of the 14 entry points from either library, which must be equal (these kernels add in a fixed order),
         at the shape lists tests/test_gpu_dwconv.py, tests/test_gpu_encoder_kernels.py and tests/test_gpu_stem.py use (read from their
         parametrize marks and from tests/encoder_kernels_oracle.py);
  bench  the per-shape calls of tools/time_dw.py, srbh_dwconv_eval_fwd at the same shapes (10 launches per graph replay) and the eval-mode
         encoder at B = 128 (tools/time_enc_eval.py): every side warmed up, --rounds alternations (the side that goes first alternates too),
         per line the rounds' medians, their median and the verdict -- the tree's median must not lie above the parent's by more than the
         parent's own spread (largest minus smallest round median); then bench.py --workload train / predict with either library through
         SRBH_LIB_PATH, alternated three times, same verdict on ms per step."""
import argparse
import ctypes
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_dw as TD  # noqa: E402
from srbh_amd import _lib  # noqa: E402
from srbh_amd import encoders as E  # noqa: E402
from tests import encoder_kernels_oracle as O  # noqa: E402
from tests import test_gpu_dwconv as T_DW  # noqa: E402
from tests import test_gpu_encoder_kernels as T_ENC  # noqa: E402
from tests import test_gpu_stem as T_STEM  # noqa: E402

DEV = "cuda:0"
SIDES = ("parent", "tree")
LIBS = {}


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def use(side):
    _lib._lib = LIBS[side]
    return LIBS[side]


def cases(test_fn):
    """the cases of a test's parametrize marks as {argument name: value} (several marks: their product)"""
    out = [{}]
    for m in test_fn.pytestmark:
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")]
        out = [dict(o, **dict(zip(names, c if len(names) > 1 else (c,)))) for o in out for c in m.args[1]]
    return out


def digest(t):
    if not torch.is_tensor(t):
        return "int %d" % t
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def show(case):
    return " ".join("%s=%s" % (k, str(v).replace(" ", "")) for k, v in case.items()) if isinstance(case, dict) else str(case)


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- one function per entry point family: returns {output name: tensor or int} from the library in use ----
def dw_direct(case):
    B, C, H, W, K, stride = case
    L = _lib.lib()
    pad, OH, OW = O.same_geometry(H, W, K, stride)
    g = torch.Generator().manual_seed(B * 7919 + C * 31 + H * 5 + K + stride)
    x, w = torch.randn((B, C, H, W), generator=g).to(DEV), (torch.randn((C, 1, K, K), generator=g) * 0.3).to(DEV)
    gy = torch.randn((B, C, OH, OW), generator=g).to(DEV)
    y, dx, dw = torch.empty_like(gy), torch.empty_like(x), torch.empty_like(w)
    splits = L.srbh_dwconv_bwd_weight_splits(B, C)
    ws = torch.full((splits * C * K * K,), float("nan"), device=DEV)
    geo = (B, C, H, W, K, stride, pad[2], pad[0], OH, OW, _lib.stream_ptr())
    _lib.check(L.srbh_dwconv_fwd(ptr(x), ptr(w), ptr(y), *geo), "dwconv_fwd")
    _lib.check(L.srbh_dwconv_bwd_data(ptr(gy), ptr(w), ptr(dx), *geo), "dwconv_bwd_data")
    _lib.check(L.srbh_dwconv_bwd_weight(ptr(x), ptr(gy), ptr(dw), ptr(ws), *geo), "dwconv_bwd_weight")
    return {"y": y, "dx": dx, "dw": dw, "splits": splits, "eval_supported": L.srbh_dwconv_eval_supported(*geo[:-1])}


def dw_autograd(case):
    K, stride, H, pad = (case[k] for k in ("K", "stride", "H", "pad"))
    g = torch.Generator().manual_seed(K * 100 + stride * 10 + H)
    B, C, W = 5, 37, H + (1 if H > 4 else 0)
    x = torch.randn((B, C, H, W), generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn((C, 1, K, K), generator=g) * 0.3).to(DEV).requires_grad_(True)
    y = E._DepthwiseConvFn.apply(x, w, stride, pad)
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    return {"y": y, "dx": x.grad, "dw": w.grad}


def dw_eval(case):
    pre, B, C, H, K, stride = (case[k] for k in ("pre", "B", "C", "H", "K", "stride"))
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 131 + C)
    x = torch.randn((B, C, H, H), generator=g).to(DEV)
    w = (torch.randn((C, 1, K, K), generator=g) * 0.3).to(DEV)
    a0, b0, a1, b1 = [(torch.rand(C, generator=g) + 0.5).to(DEV) if i % 2 == 0 else (torch.randn(C, generator=g) * 0.2).to(DEV) for i in range(4)]
    OH = math.ceil(H / stride)
    pt = max((OH - 1) * stride + K - H, 0) // 2
    y, pooled = torch.empty((B, C, OH, OH), device=DEV), torch.empty((B, C), device=DEV)
    _lib.check(L.srbh_dwconv_eval_fwd(ptr(x), ptr(w), ptr(a0) if pre else None, ptr(b0) if pre else None, ptr(a1), ptr(b1), ptr(y), ptr(pooled),
                                      B, C, H, H, K, stride, pt, pt, OH, OH, _lib.stream_ptr()), "dwconv_eval_fwd")
    return {"y": y, "pooled": pooled, "eval_supported": L.srbh_dwconv_eval_supported(B, C, H, H, K, stride, pt, pt, OH, OH)}


def affine(case):
    B, C, HW, act, with_res = case
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + act)
    x, scale, shift, res = [None if t is None else t.to(DEV) for t in T_ENC._affine_inputs(B, C, HW, g, with_res)]
    y = torch.empty_like(x)
    T_ENC._affine_call(_lib.lib(), x, scale, shift, res, y, B, C, HW, act)
    return {"y": y}


def affine_pool(case):
    HW, B, C, act = (case[k] for k in ("HW", "B", "C", "act"))
    g = torch.Generator().manual_seed(HW * 7 + B * C + act)
    x, scale, shift, _ = [None if t is None else t.to(DEV) for t in T_ENC._affine_inputs(B, C, HW, g, False)]
    y, pooled = torch.empty_like(x), torch.empty((B, C), device=DEV)
    _lib.check(_lib.lib().srbh_affine_act_pool_nchw(ptr(x), ptr(scale), ptr(shift), ptr(y), ptr(pooled), B, C, HW, act, _lib.stream_ptr()), "affine_act_pool_nchw")
    return {"y": y, "pooled": pooled}


def se_hidden(case):
    B, SQ, C = (case[k] for k in ("B", "SQ", "C"))
    g = torch.Generator().manual_seed(C * 31 + SQ * 7 + B)
    pooled = (torch.randn((B, C), generator=g) * 0.5 + 0.3).to(DEV)
    w1, b1 = [t.to(DEV) for t in T_ENC._se_weights(SQ, C, g)]
    hidden = torch.empty((B, SQ), device=DEV)
    _lib.check(_lib.lib().srbh_se_hidden(ptr(pooled), ptr(w1), ptr(b1), ptr(hidden), B, C, SQ, _lib.stream_ptr()), "se_hidden")
    return {"hidden": hidden}


def se_gate(case):
    B, C, SQ = (case[k] for k in ("B", "C", "SQ"))
    g = torch.Generator().manual_seed(B * 977 + C * 13 + SQ)
    hidden = F.silu(torch.randn((B, SQ), generator=g)).to(DEV)
    w2, b2 = [t.to(DEV) for t in T_ENC._se_weights(C, SQ, g)]
    gate = torch.empty((B, C), device=DEV)
    _lib.check(_lib.lib().srbh_se_gate(ptr(hidden), ptr(w2), ptr(b2), ptr(gate), B, C, SQ, _lib.stream_ptr()), "se_gate")
    return {"gate": gate}


def se_gate_scale(case):
    B, C, SQ, HW, offset = (case.get(k, d) for k, d in (("B", 3), ("C", 5), ("SQ", None), ("HW", None), ("offset", 0)))
    g = torch.Generator().manual_seed(B * 977 + C * 13 + SQ * 3 + HW)
    y0 = F.silu(torch.randn((B, C, HW), generator=g) * 1.5 + 0.4)
    hidden = F.silu(torch.randn((B, SQ), generator=g)).to(DEV)
    w2, b2 = [t.to(DEV) for t in T_ENC._se_weights(C, SQ, g)]
    buf = torch.zeros(y0.numel() + 4, device=DEV)
    y = buf[offset:offset + y0.numel()].view(y0.shape)          # offset 1: one float past a 16-byte boundary -> the wave-per-plane kernel
    y.copy_(y0)
    _lib.check(_lib.lib().srbh_se_gate_scale(ptr(y), ptr(hidden), ptr(w2), ptr(b2), B, C, SQ, HW, _lib.stream_ptr()), "se_gate_scale")
    return {"y": y}


def stem(case):
    B, Cin, Cout, H, W, size = (case[k] for k in ("B", "Cin", "Cout", "H", "W", "size"))
    torch.manual_seed(B + Cin)
    conv = E.SamePadConv2d(Cin, Cout, 3, size, stride=2, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(Cout, momentum=E.BN_MOM, eps=E.BN_EPS).to(DEV).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3); bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
        x = torch.randn((B, Cin, H, W), device=DEV)
        return {"y": E._stem_eval(conv, bn, x), "stem_supported": _lib.lib().srbh_stem_conv_eval_supported(Cin, Cout, 3)}


def bit_cases():
    dw = [c for c, _ in O.DW_SLICE_CASES] + [c for c, _ in O.DW_LIMIT_CASES] + [O.DW_WRAP_CASE]
    quad = [dict(c, offset=off) for c in cases(T_ENC.test_se_gate_scale_quad_planes) for off in (0, 1)]          # (B, C = 3, 5 as the test has them)
    return [("dwconv fwd / bwd_data / bwd_weight B C H W K s", dw_direct, dw),
            ("dwconv autograd", dw_autograd, cases(T_DW.test_depthwise_conv_matches_stock_op)),
            ("dwconv_eval_fwd", dw_eval, cases(T_DW.test_fused_inference_depthwise_bn_swish_pool_kernel)),
            ("affine_act(_add) B C HW act res", affine, [(B, C, HW, act, res) for B, C, HW in T_ENC.AFFINE_SHAPES for act in (0, 1, 2) for res in (False, True)]),
            ("affine_act_pool", affine_pool, cases(T_ENC.test_affine_act_pool_matches_the_oracle)),
            ("se_hidden", se_hidden, cases(T_ENC.test_se_hidden_matches_the_oracle)),
            ("se_gate", se_gate, cases(T_ENC.test_se_gate_matches_the_oracle)),
            ("se_gate_scale", se_gate_scale, quad + cases(T_ENC.test_se_gate_scale_other_planes)),
            ("stem_conv_eval", stem, cases(T_STEM.test_stem_kernel_against_the_float64_chain))]


def bits(rows):
    ok, n = True, 0
    for title, fn, lst in bit_cases():
        for case in lst:
            d = {}
            for side in SIDES:
                use(side)
                d[side] = {k: digest(v) for k, v in fn(case).items()}
                torch.cuda.synchronize()
            for k in d["parent"]:
                same = d["parent"][k] == d["tree"][k]
                ok &= same
                n += 1
                rows.append("%-48s %-62s %-14s %s %s %s" % (title, show(case), k, d["parent"][k], d["tree"][k], "equal" if same else "DIFFERENT"))
                print(rows[-1], flush=True)
    rows.append("%d outputs: %s" % (n, "ALL EQUAL" if ok else "SOME DIFFER"))
    print(rows[-1], flush=True)
    return ok


def verdict(rows, name, med, unit):
    p, t = statistics.median(med["parent"]), statistics.median(med["tree"])
    spread = max(med["parent"]) - min(med["parent"])
    ok = t <= p + spread
    rows += ["%s" % name,
             "   parent rounds: %s" % " ".join("%.3f" % x for x in med["parent"]),
             "   tree rounds:   %s" % " ".join("%.3f" % x for x in med["tree"]),
             "   parent %.3f %s, tree %.3f %s (%+.2f %%), parent's spread %.3f %s (%.2f %%): %s"
             % (p, unit, t, unit, 100 * (t - p) / p, spread, unit, 100 * spread / p, "PASS" if ok else "FAIL")]
    print("\n".join(rows[-4:]), flush=True)
    return ok


def bench_line(rows, name, make, sample, samples, rounds, unit):
    """make(): the side's warmed-up graph, built with that side's library in use; sample(graph): one timing"""
    graphs = {}
    for side in SIDES:
        use(side)
        graphs[side] = make()
    med = {s: [] for s in SIDES}
    for r in range(rounds):
        for side in (SIDES if r % 2 == 0 else SIDES[::-1]):
            med[side].append(statistics.median(sample(graphs[side]) for _ in range(samples)))
    return verdict(rows, name, med, unit)


def eval_call(c):
    B, C, H, _, K, s, pt, pl, OH, _ = c["geo"]
    a0, b0, a1, b1 = [torch.rand(C, device=DEV) + 0.5 if i % 2 == 0 else torch.randn(C, device=DEV) * 0.2 for i in range(4)]
    pooled = torch.empty((B, C), device=DEV)
    return lambda: _lib.check(_lib.lib().srbh_dwconv_eval_fwd(ptr(c["x"]), ptr(c["w"]), ptr(a0), ptr(b0), ptr(a1), ptr(b1), ptr(c["y"]), ptr(pooled),
                                                            *c["geo"], _lib.stream_ptr()), "dwconv_eval_fwd")


def replays_ms(g, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench_encoder(rows, rounds):
    """The eval-mode encoder at B = 128 as one graph (tools/time_enc_eval.py).  A captured graph owns its intermediates, and two graphs of the SAME
    library replay up to 0.5 % apart depending on where theirs lie (measured with the parent's library on both sides); so every round captures the
    side's graph anew into one memory pool, where it gets the addresses the other side's graph just gave back, times it and drops it."""
    torch.manual_seed(0)
    enc = E.get_encoder("efficientnet-b4", in_channels=8, depth=5, weights=None).cuda().eval()
    x = torch.rand((128, 8, 64, 64), device="cuda")
    pool = torch.cuda.graph_pool_handle()
    anchor = torch.cuda.CUDAGraph()                       # keeps the pool alive between the sides' graphs
    with torch.cuda.graph(anchor, pool=pool):
        held = torch.zeros(64, device="cuda")
    med = {s: [] for s in SIDES}
    with torch.no_grad():
        for side in SIDES:                                # every side warmed up
            use(side)
            for _ in range(3):
                enc(x)
        torch.cuda.synchronize()
        for r in range(rounds):
            for side in (SIDES if r % 2 == 0 else SIDES[::-1]):
                use(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    out = enc(x)
                g.replay(); torch.cuda.synchronize()
                med[side].append(statistics.median(replays_ms(g) for _ in range(3)))
                del g, out
    del anchor, held
    return verdict(rows, "EfficientNet-B4 encoder, eval mode, B=128, one graph replay (captured anew every round into one pool)", med, "ms")


def bench_py(rows, libs, workload, extra):
    """bench.py in a fresh process per run with either library through SRBH_LIB_PATH, alternated three times; ms per step"""
    med, tiles = {s: [] for s in SIDES}, {s: [] for s in SIDES}
    for r in range(3):
        for side in (SIDES if r % 2 == 0 else SIDES[::-1]):
            env = dict(os.environ, SRBH_LIB_PATH=libs[side])
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, *extra], env=env, cwd=ROOT,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert out.returncode == 0, out.stdout[-2000:]
            line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
            med[side].append(line["ms_per_step"])
            tiles[side].append(line["value"])
            print("bench.py %s %s: %.3f ms per step, %.1f tiles/s" % (workload, side, line["ms_per_step"], line["value"]), flush=True)
    ok = verdict(rows, "bench.py --gpus 1 --workload %s %s, ms per step of each run" % (workload, " ".join(extra)), med, "ms")
    rows.append("   tiles/s: parent %s; tree %s" % (" ".join("%.1f" % v for v in tiles["parent"]), " ".join("%.1f" % v for v in tiles["tree"])))
    return ok


def bench(rows, rounds, libs, with_bench_py, only_encoder=False):
    ok = True
    for C, H, K, s in ([] if only_encoder else TD.shapes):
        use("tree")
        c = TD.calls(C, H, K, s)
        tag = "B=%d C=%d %dx%d K=%d s=%d" % (TD.B, C, H, H, K, s)
        for name, fn in (("srbh_dwconv_fwd", c["fwd"]), ("srbh_dwconv_bwd_data", c["bwd_data"]), ("srbh_dwconv_bwd_weight (+ reduce)", c["bwd_weight"]),
                         ("srbh_dwconv_eval_fwd", eval_call(c))):
            ok &= bench_line(rows, "%-34s %s" % (name, tag), lambda: TD.graph_of(fn), TD.replay_us, 5, rounds, "us")
    ok &= bench_encoder(rows, rounds)
    if with_bench_py:
        ok &= bench_py(rows, libs, "train", ("--steps", "30", "--warmup", "5", "--no-cpu-baseline", "--no-extras"))
        ok &= bench_py(rows, libs, "predict", ("--steps", "12", "--no-extras"))
    rows.append("ALL PASS" if ok else "SOME FAIL")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--tree-lib", default=_lib.LIB_PATH, help="the library on the tree's side (the parent's again: a control of the method)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bits-out", default=os.path.join(ROOT, "profiles", "dw_pieces_bits.txt"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "dw_pieces_bench.txt"))
    ap.add_argument("--only", choices=["bits", "bench"], default=None)
    ap.add_argument("--only-encoder", action="store_true", help="bench part: the encoder line alone")
    ap.add_argument("--no-bench-py", action="store_true", help="leave out the bench.py runs at the end of the bench part")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    parent_lib = os.path.abspath(args.parent_lib)
    tree_lib = os.path.abspath(args.tree_lib)
    LIBS["parent"], LIBS["tree"] = load(parent_lib), load(tree_lib)
    prop = torch.cuda.get_device_properties(0)
    dev = "device %s (%s, %d CUs); torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                        torch.__version__, torch.version.hip)
    ok = True
    for part, out, head in (("bits", args.bits_out, "Depthwise conv and encoder inference kernels, parent library against this tree's: sha256 (first 16 hex "
                             "digits) of every output buffer, parent then tree; " + dev),
                            ("bench", args.bench_out, "Depthwise conv and encoder inference kernels, parent library against this tree's in one process, "
                             "%d alternations; us per launch (10 launches per graph replay, median of 5 samples per round), the encoder in ms per "
                             "replay; " % args.rounds + dev)):
        if args.only in (None, part):
            rows = [head, ""]
            ok &= (bits if part == "bits" else lambda r: bench(r, args.rounds, {"parent": parent_lib, "tree": tree_lib}, not args.no_bench_py, args.only_encoder))(rows)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as fh:
                fh.write("\n".join(rows) + "\n")
            print("wrote", out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
