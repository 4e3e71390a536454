"""Do the dense attention backward kernels still compile to the instructions another revision gave them?

od_flash_attn_bwd_varlen added a VL template flag to flash_bwd_dkv_kernel, flash_bwd_dq_kernel and attn_delta_kernel.  This tool compiles
osu_dreamer_amd/csrc/attn.hip of the working tree and of a git revision to gfx950 assembly (device code only, build.sh's flags for attn*.hip),
pairs every kernel of the revision with the instantiation of the same template arguments in the working tree (with `, false` appended where
the tree has one more flag), and compares their instruction streams with comments, directives and block-label numbers removed.
Exit status 0: every paired kernel is identical.  Needs hipcc and c++filt; no GPU.

  python tools/dense_isa_diff.py [--rev HEAD~1] [--kernels flash_bwd_dkv,flash_bwd_dq,attn_delta]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("osu_dreamer_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffinite-math-only", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
DEPS = ["attn.hip", "od_common.h", "od_tiles.h", "od_api_internal.h"]


def stage(top, rev):
    """csrc/ and include/ of `rev` (None: the working tree) under `top`, at the depths the sources' relative includes expect."""
    cs, inc = os.path.join(top, "a", "b"), os.path.join(top, "include")
    os.makedirs(cs)
    os.makedirs(inc)
    for rel, dst in [(os.path.join(CSRC, f), os.path.join(cs, f)) for f in DEPS] + [("include/osu_dreamer_hip.h", os.path.join(inc, "osu_dreamer_hip.h"))]:
        if rev is None:
            shutil.copy(os.path.join(ROOT, rel), dst)
        else:
            with open(dst, "wb") as f:
                f.write(subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:{rel}"]))
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, "attn.hip", "-o", "attn.s"], cwd=cs, stderr=subprocess.DEVNULL)
    return os.path.join(cs, "attn.s")


def kernels(path, wanted):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                if any(w in name for w in wanted):
                    out[name] = body
                name = None
                continue
            t = re.sub(r";.*$", "", line).strip()
            if t and not t.startswith("."):
                body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")

    def key(s):
        s = s.replace("(anonymous namespace)::", "").replace("void ", "", 1)
        return s[:s.index(">(") + 1] if ">(" in s else s
    return {key(d): out[n] for n, d in zip(names, dem)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD~1")
    ap.add_argument("--kernels", default="flash_bwd_dkv,flash_bwd_dq,attn_delta")
    a = ap.parse_args()
    wanted = a.kernels.split(",")
    with tempfile.TemporaryDirectory() as top:
        old = kernels(stage(os.path.join(top, "old"), a.rev), wanted)
        new = kernels(stage(os.path.join(top, "new"), None), wanted)
    same = diff = 0
    for name, body in sorted(old.items()):
        nb = new.get(name) or new.get(name[:-1] + ", false>")
        if nb == body:
            same += 1
        else:
            diff += 1
            print(f"DIFFERENT {name}: {len(body)} instructions in {a.rev}, {len(nb) if nb else 'no such kernel'} in the working tree")
    print(f"{same} dense kernels identical to {a.rev}, {diff} different, of {len(old)}")
    return 1 if diff or not old else 0


if __name__ == "__main__":
    sys.exit(main())
