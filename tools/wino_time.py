"""Dev tool: time skp_conv3x3_wino forward on a few shapes (TF/s-equivalent of the direct conv).

usage: python tools/wino_time.py [--shapes B,C,K,HW;...]  (timing-probe builds: tools/build_variant.sh with -DSKP_WINO_DEBUG=… / -DSKP_WINO2_DEBUG=…)

       python tools/wino_time.py --pair "B,C,K,HW;..." [--repeats 3]
           A/B of the gradient-free GroupNorm + SiLU → 3×3 convolution pair (the VAE resnets' conv2
           form: shift, bias and residual): "old" = gn_apply + wino2 (ops.group_norm_act +
           ops.conv3x3), "new" = vtransform_gn + wino2_v (ops.gn_conv3x3).  Each measurement runs in
           a process of its own (--side), HIP events around --iters back-to-back pairs; the sides
           alternate --repeats times.  A shape passes where every new repeat is below every old one
           (the gate of ops.WINO_V_SHAPES).

       python tools/wino_time.py --kernels "B,C,K,HW;..." [--libs A.so,B.so] [--repeats 3]
           The two kernels of the new pair timed apart, straight through the C entry points:
           "vtrans" = skp_wino2_vtransform_gn (GroupNorm + SiLU + shift), "vconv" =
           skp_conv3x3_wino2_v_gn (bias, residual, statistics partials).  One process per
           measurement (--side vtrans|vconv); with --libs the libraries alternate (SKP_LIB), so a
           library built from another revision (tools/build_rev.sh) is compared kernel by kernel.
           V is allocated at 40 floats per tile, enough for either layout.
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="8,128,128,512;8,512,512,128;8,512,512,64;8,320,320,64;8,640,640,32;8,1280,1280,16")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--residual", action="store_true", help="bias + residual epilogue (the resnet conv2 form)")
ap.add_argument("--pair", default="", help="B,C,K,HW;...: A/B the GroupNorm → conv pair, one process per side")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--kernels", default="", help="B,C,K,HW;...: time vtransform_gn and wino2_v apart, one process each")
ap.add_argument("--libs", default="", help="comma-separated libskp.so paths to alternate under --kernels (default: the tree's)")
ap.add_argument("--side", default="", choices=["", "old", "new", "vtrans", "vconv"],
                help="(internal) one side of --pair / --kernels, one shape")
a = ap.parse_args()

if a.pair and not a.side:
    for s in a.pair.split(";"):
        res = {"old": [], "new": []}
        for _ in range(a.repeats):
            for side in ("old", "new"):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pair", s, "--side", side,
                                      "--iters", str(a.iters)], check=True, capture_output=True, text=True, timeout=300).stdout
                res[side].append(float(out.split()[-2]))
        old, new = res["old"], res["new"]
        gain = 1 - sorted(new)[len(new) // 2] / sorted(old)[len(old) // 2]
        print(f"pair {s}: old us {' '.join(f'{t:.1f}' for t in old)} | new us {' '.join(f'{t:.1f}' for t in new)} | "
              f"median gain {100 * gain:+.1f}% | {'PASS' if max(new) < min(old) else 'no'}", flush=True)
    sys.exit(0)

if a.kernels and not a.side:
    libs = a.libs.split(",") if a.libs else [""]
    for s in a.kernels.split(";"):
        for side in ("vconv", "vtrans"):
            res = {lib: [] for lib in libs}
            for _ in range(a.repeats):
                for lib in libs:
                    env = dict(os.environ, **({"SKP_LIB": os.path.abspath(lib)} if lib else {}))
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pair", s, "--side", side,
                                          "--iters", str(a.iters)], check=True, capture_output=True, text=True, timeout=300,
                                         env=env).stdout
                    res[lib].append(float(out.split()[-2]))
            line = " | ".join(f"{lib or 'tree'} us {' '.join(f'{t:.1f}' for t in ts)}" for lib, ts in res.items())
            verdict = ""
            if len(libs) == 2:
                old, new = res[libs[0]], res[libs[1]]
                gain = 1 - sorted(new)[len(new) // 2] / sorted(old)[len(old) // 2]
                verdict = f" | median gain {100 * gain:+.1f}% | {'PASS' if max(new) < min(old) else 'no'}"
            print(f"{side} {s}: {line}{verdict}", flush=True)
    sys.exit(0)

import torch  # noqa: E402
from stablekeypoints_amd import ops  # noqa: E402


def timed(f, iters):
    f()
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


if a.side:
    B, C, K, HW = map(int, a.pair.split(","))
    dev = "cuda:0"
    torch.manual_seed(0)
    with torch.no_grad():
        # x comes out of a convolution, so it carries its GroupNorm statistics partials as in the VAE
        x = ops.conv3x3(torch.randn(B, 4, HW, HW, device=dev), torch.randn(C, 4, 3, 3, device=dev) / 6)
        w = torch.randn(K, C, 3, 3, device=dev) / (3 * C ** 0.5)
        gamma, beta = 1 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
        shift, bias = 0.1 * torch.randn(1, C, device=dev), torch.randn(K, device=dev)
        r = torch.randn(B, K, HW, HW, device=dev)
        if a.side in ("vtrans", "vconv"):
            from stablekeypoints_amd._lib import call, ptr, stream
            st = stream(torch.device(dev))
            part = torch.empty(ops._lib.lib().skp_groupnorm_workspace(B, C, HW * HW, 32), device=dev, dtype=torch.float64)
            stats = torch.empty(B * 32 * 2, device=dev)
            sh = shift.expand(B, C).contiguous()
            call("skp_groupnorm_stats", ptr(x), ptr(sh), B, C, HW * HW, 32, 1e-6, ptr(stats), ptr(part), st)
            V = torch.zeros(B * C * (HW // 4) * (HW // 4) * 40, device=dev)
            U = ops._wino_u(w, False, True)
            y = torch.empty(B, K, HW, HW, device=dev)
            gnp = torch.empty(B, K, (HW // 16) * (HW // 32), 2, device=dev)
            ftrans = lambda: call("skp_wino2_vtransform_gn", ptr(x), ptr(stats), ptr(gamma), ptr(beta), ptr(sh), 32, 1,
                                  ptr(V), B, C, HW, HW, st)
            ftrans()
            if a.side == "vtrans":
                f = ftrans
            else:
                f = lambda: call("skp_conv3x3_wino2_v_gn", ptr(V), ptr(U), ptr(bias), ptr(r), ptr(y), B, C, K, HW, HW, 1,
                                 None, ptr(gnp), st)
        elif a.side == "old":
            f = lambda: ops.conv3x3(ops.group_norm_act(x, gamma, beta, 32, 1e-6, True, shift), w, bias, r)
        else:
            f = lambda: ops.gn_conv3x3(x, gamma, beta, 32, 1e-6, True, shift, w, bias, r)
        t = timed(f, a.iters)
    print(f"{a.side} {B}x{C}->{K} {HW}^2: {t * 1e3:.1f} us", flush=True)
    sys.exit(0)

for s in a.shapes.split(";"):
    B, C, K, HW = map(int, s.split(","))
    x = torch.randn(B, C, HW, HW, device="cuda:0")
    w = torch.randn(K, C, 3, 3, device="cuda:0") / (3 * C ** 0.5)
    b = torch.randn(K, device="cuda:0") if a.residual else None
    r = torch.randn(B, K, HW, HW, device="cuda:0") if a.residual else None
    f = lambda: ops._wino_conv(x, w, False, b, r, K)
    t = timed(f, a.iters)
    fl = 2 * B * HW * HW * C * K * 9
    print(f"{B}x{C}->{K} {HW}^2: {t * 1e3:8.1f} us  {fl / (t * 1e-3) / 1e12:6.1f} TF/s-equiv  "
          f"({fl / 4 / (t * 1e-3) / 1e12:5.1f} TF/s MFMA)", flush=True)
