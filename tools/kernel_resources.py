"""Dev tool: the register, scratch and occupancy figures of every kernel of one HIP source, as a table.

Compiles the file for gfx950 with the library's flags and ``-Rpass-analysis=kernel-resource-usage``
(no GPU needed) and prints one row per kernel, sorted by name: the demangled kernel with its template
arguments and without its parameter list (so a row can be compared between two trees when only a
kernel's parameters changed), then SGPRs, VGPRs, AGPRs, scratch bytes per lane, waves per SIMD and
LDS bytes.  Two trees compile to the same kernels where their tables' rows are the same.

Usage: python tools/kernel_resources.py stablekeypoints_amd/csrc/skp_tta.hip [--out FILE]
"""
import argparse
import os
import re
import subprocess
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-munsafe-fp-atomics",
         "-Rpass-analysis=kernel-resource-usage"]
FIELDS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch_B"),
          ("Occupancy [waves/SIMD]", "waves_per_SIMD"), ("LDS Size [bytes/block]", "LDS_B"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = []
    for full in out[:len(names)]:
        full = re.sub(r"^void ", "", full).replace("(anonymous namespace)::", "")
        depth = 0
        for at, ch in enumerate(full):      # cut at the parameter list: the first '(' outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                full = full[:at]
                break
        short.append(full)
    return short


def table(source):
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([HIPCC, *FLAGS, "-c", source, "-o", os.path.join(tmp, "o.o")], capture_output=True, text=True,
                             check=True, cwd=os.path.dirname(os.path.abspath(source))).stderr
    kernels, cur = [], None
    for line in err.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            kernels.append(cur)
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    for k, short in zip(kernels, demangle([k["name"] for k in kernels])):
        k["short"] = short
    rows = [[k["short"]] + [k.get(f, "?") for f, _ in FIELDS] for k in sorted(kernels, key=lambda k: k["short"])]
    head = ["kernel"] + [h for _, h in FIELDS]
    width = [max(len(r[c]) for r in [head] + rows) for c in range(len(head))]
    return "\n".join("  ".join(v.ljust(w) for v, w in zip(r, width)).rstrip() for r in [head] + rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = table(os.path.abspath(a.source))
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
