"""developer aid: device time of the depthwise kernels per EfficientNet-B4 shape (batch 64), 10 launches per graph replay, through the C ABI.
usage: [SRBH_LIB_PATH=variant.so] python tools/time_dw.py     (tools/ab_encoder_kernels.py imports shapes, calls and timed)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srbh_amd import _lib
dev, B = "cuda:0", 64
shapes = [(48, 32, 3, 1), (144, 32, 3, 2), (192, 16, 3, 1), (192, 16, 5, 2), (336, 8, 5, 1), (336, 8, 3, 2), (672, 4, 3, 1), (672, 4, 5, 1), (960, 4, 5, 2), (1632, 2, 5, 1), (2688, 2, 3, 1)]


def graph_of(fn):
    """fn warmed up on a side stream, then 10 launches of it captured as one graph"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    """us per launch over 10 replays of a graph_of() graph"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 100 * 1e3


def timed(fn):
    return replay_us(graph_of(fn))


def calls(C, H, K, s):
    """{name: call} of the three depthwise entry points at one shape, on the library _lib.lib() returns when the call runs"""
    pl, pr, pt, pb = {(3, 1): (1, 1, 1, 1), (3, 2): (0, 1, 0, 1), (5, 1): (2, 2, 2, 2), (5, 2): (1, 2, 1, 2)}[(K, s)]
    OH = (H + pt + pb - K) // s + 1
    x = torch.randn(B, C, H, H, device=dev); w = torch.randn(C, 1, K, K, device=dev)
    y = torch.empty(B, C, OH, OH, device=dev); dy = torch.randn_like(y); dx = torch.empty_like(x); dw = torch.empty_like(w)
    ws = torch.empty(_lib.lib().srbh_dwconv_bwd_weight_splits(B, C) * C * K * K, device=dev)
    geo = (B, C, H, H, K, s, pt, pl, OH, OH)
    return {"geo": geo, "x": x, "w": w, "y": y,
            "fwd": lambda: _lib.check(_lib.lib().srbh_dwconv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), *geo, _lib.stream_ptr())),
            "bwd_data": lambda: _lib.check(_lib.lib().srbh_dwconv_bwd_data(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), *geo, _lib.stream_ptr())),
            "bwd_weight": lambda: _lib.check(_lib.lib().srbh_dwconv_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), *geo, _lib.stream_ptr()))}


if __name__ == "__main__":
    for C, H, K, s in shapes:
        c = calls(C, H, K, s)
        f, d, g = timed(c["fwd"]), timed(c["bwd_data"]), timed(c["bwd_weight"])
        print(f"C={C:5d} {H:2d}x{H:<2d} K={K} s={s}: fwd {f:6.1f}  bwd_data {d:6.1f}  bwd_weight(+reduce) {g:6.1f} us", flush=True)
