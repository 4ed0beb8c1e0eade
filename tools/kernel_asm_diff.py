#!/usr/bin/env python3
"""Compare the device code of two source trees kernel by kernel, without a GPU.

    python tools/kernel_asm_diff.py TREE_A TREE_B

Every csrc/*.hip of both trees is compiled to gfx950 device assembly with the Makefile's flags plus
`--cuda-device-only -S`.  The output is split per kernel symbol, comments are dropped and local labels are
renumbered in order of appearance, and per file the kernels are reported as added, removed, identical or
differing.  It compares text and nothing else.  Exit status 1 if any kernel was added, removed or differs.
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("naqs-for-quantum-chemistry_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# csrc/Makefile: CXXFLAGS
FLAGS = "-O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off".split()


def compile_asm(tree, name, out_dir):
    inc = tempfile.mkdtemp(dir=out_dir)
    with open(os.path.join(inc, "naqs_src_hash.h"), "w") as f:      # (host-only: the same for both trees)
        f.write('#define NAQS_SRC_HASH "0"\n')
    out = os.path.join(inc, name + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", *FLAGS, "-I" + os.path.join(tree, "include"), "-I" + inc,
           "--cuda-device-only", "-S", "-o", out, os.path.join(tree, CSRC, name)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def kernels(asm):
    """kernel symbol -> normalised text of its body (from its label to its .Lfunc_end)."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    out, cur, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if cur is None:
            if m and m.group(1) in names:
                cur, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[cur] = normalise(body)
            cur = None
            continue
        body.append(line)
    return out


def normalise(lines):
    text = []
    for line in lines:
        line = re.sub(r"\s*;.*$", "", line).strip()
        if line and not line.startswith((".loc", ".file", ".cfi_", ".p2align")):
            text.append(line)
    labels = {}
    def renum(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    return "\n".join(re.sub(r"\.L[\w$.]+", renum, line) for line in text)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = (os.path.abspath(t) for t in sys.argv[1:])
    files = sorted(set(f for t in (a, b) for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")))
    bad = False
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        jobs = {(t, f): pool.submit(compile_asm, t, f, tmp) for t in (a, b) for f in files
                if os.path.exists(os.path.join(t, CSRC, f))}
        for f in files:
            ka = kernels(jobs[(a, f)].result()) if (a, f) in jobs else {}
            kb = kernels(jobs[(b, f)].result()) if (b, f) in jobs else {}
            added, removed = sorted(set(kb) - set(ka)), sorted(set(ka) - set(kb))
            differing = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            same = len(set(ka) & set(kb)) - len(differing)
            print("%-22s %3d kernels -> %3d   identical %d, differing %d, added %d, removed %d"
                  % (f, len(ka), len(kb), same, len(differing), len(added), len(removed)))
            for tag, ks in (("differs", differing), ("added", added), ("removed", removed)):
                for k in ks:
                    print("    %-8s %s" % (tag, k))
            bad = bad or bool(added or removed or differing)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
