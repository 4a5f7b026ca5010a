"""Timing of the VAE's stride-2 downsampling convolutions at the bench batch (8 = 4 images + 4
warps), three ways: "f2" (skp_conv3x3s2_f2, 25 products per 2×2 tile), "miopen" (the edge-pad copy +
MIOpen conv2d(stride 2), what Downsample2D runs when the fused path is off) and "sampled"
(skp_conv3x3s2_wino2, the stride-1 F(4×4, 3×3) kernel sampled at the odd rows / columns, which
skp_conv3x3s2_f2 replaced: timed only when SKP_OLD_LIB names a library built from a revision that
still has it, e.g. by tools/build_rev.sh).  Dev tool.

  python tools/conv_s2_time.py                 three alternating repeats of every method at the three
                                               bench shapes, each measurement in a process of its own
  python tools/conv_s2_time.py METHOD C H      one measurement: prints microseconds per call
"""
import os
import subprocess
import sys

SHAPES = ((128, 512), (256, 256), (512, 128))
METHODS = (("sampled",) if os.environ.get("SKP_OLD_LIB") else ()) + ("f2", "miopen")


def timed(fn, iters=20):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def one(method, C, H):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from stablekeypoints_amd import ops
    from stablekeypoints_amd.sd.unet import Downsample2D
    m = Downsample2D(C, padding=0).to("cuda")
    for p in m.parameters():
        p.requires_grad_(False)
    x = torch.randn(8, C, H, H, device="cuda")
    ops.WINO_S2_MIN_PIXELS = 1
    fn = lambda: m(x)
    if method == "miopen":
        ops.WINO_S2 = False
    elif method == "sampled":
        import ctypes
        old = ctypes.CDLL(os.environ["SKP_OLD_LIB"])
        U = ops._wino_u(m.conv.weight, False, True)
        y = torch.empty(8, C, H // 2, H // 2, device="cuda")
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = lambda: old.skp_conv3x3s2_wino2(P(x), P(U), P(m.conv.bias), P(y), 8, C, C, H, H, 1, None, st)
    with torch.no_grad():
        print(f"{timed(fn):.1f}", flush=True)


def main():
    rows = {(m, s): [] for m in METHODS for s in SHAPES}
    for rep in range(3):
        for s in SHAPES:
            for m in METHODS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), m, str(s[0]), str(s[1])],
                                   capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"{m} {s}: exit {r.returncode}\n{r.stderr[-2000:]}")
                rows[(m, s)].append(float(r.stdout.split()[-1]))
    for s in SHAPES:
        for m in METHODS:
            print(f"{s[0]:4d} ch {s[1]}²  {m:8s} " + "  ".join(f"{t:8.1f}" for t in rows[(m, s)]) + "  us", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4:
        one(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
