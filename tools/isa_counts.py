#!/usr/bin/env python3
"""Static instruction counts of the library's kernels from the compiler's gfx950 assembly (no GPU needed).
    python tools/isa_counts.py [source.hip] [kernel name substring ...] [--asm FILE] [--hash]   (default: voxelize_lists.hip, the two brick kernels)
    python tools/isa_counts.py --all [--usage]      (every kernel of every .hip of the build, sorted by name: name and stream hash)
Per kernel: vector ALU / scalar ALU / vector loads / vector stores + atomics / LDS instructions, and how many correctly rounded
divisions (v_div_fixup_f32) and square roots (v_sqrt_f32) it contains.  --hash: also a hash of the kernel's instruction stream (its
body without labels, comments and directives; local labels numbered in order of appearance, so a kernel that moved to another file or
position hashes the same) -- equal hashes of two builds: the same code.  --all --usage: instead of the hash, the compiler's resource
remarks of the last build (csrc/build/*.usage): VGPRs, SGPRs, LDS, scratch, occupancy."""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dxrvoxelizer_amd import build as B  # noqa: E402


def assembly(src):
    out = os.path.join(tempfile.mkdtemp(prefix="dxv_isa_"), "k.s")
    cmd = [B.hipcc()] + [f for f in B.FLAGS if not f.startswith("-W")] + ["-w", "--cuda-device-only", "-S", "-o", out, os.path.join(B.CSRC, src)]
    subprocess.check_call(cmd)
    return out


def bodies(path, wanted):
    txt = open(path).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        if any(w in m.group(1) for w in wanted) if wanted else m.group(1) in kernels:
            yield m.group(1), m.group(2)


def stream_hash(body):
    labels, out = {}, []
    for line in body.split("\n"):
        line = line.split(";")[0].rstrip()
        if re.match(r"\s+[a-z]", line):                        # an instruction (labels start in column 0, directives with a dot)
            out.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), " ".join(line.split())))
    return hashlib.sha256("\n".join(out).encode()).hexdigest()[:16], len(out)


def counts(path, wanted, hashes=False):
    res = {}
    for name, body in bodies(path, wanted):
        c = collections.Counter()
        for line in body.split("\n"):
            op = re.match(r"\s+([a-z][a-z_0-9]+)", line)
            if not op:
                continue
            op = op.group(1)
            if op.startswith("v_"):
                c["valu"] += 1
            elif op.startswith("s_"):
                c["salu"] += 1
            elif op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load")):
                c["vector_loads"] += 1
            elif op.startswith(("global_store", "global_atomic", "buffer_store", "flat_store", "scratch_store")):
                c["vector_stores"] += 1
            elif op.startswith("ds_"):
                c["lds"] += 1
            if op == "v_div_fixup_f32":
                c["divisions_f32"] += 1
            if op == "v_sqrt_f32":
                c["sqrt_f32"] += 1
            if op == "v_div_fixup_f64":
                c["divisions_f64"] += 1
        res[name] = dict(c)
        if hashes:
            res[name]["stream_sha256"], res[name]["instructions"] = stream_hash(body)
    return res


def all_kernels(usage):
    """one line per kernel of every .hip in the build's SOURCES, sorted by kernel name (file and position do not appear)"""
    rows = []                                                  # (a list: a kernel instantiated in two translation units appears twice)
    for src in (s for s in B.SOURCES if s.endswith(".hip")):
        if usage:
            rows += B.kernel_resources(os.path.splitext(src)[0]).items()
        else:
            rows += [(k, {"stream_sha256": c["stream_sha256"], "instructions": c["instructions"]}) for k, c in counts(assembly(src), [], True).items()]
    return sorted(rows, key=lambda r: (r[0], sorted(r[1].items())))


if __name__ == "__main__":
    if "--all" in sys.argv:
        import json
        for name, c in all_kernels("--usage" in sys.argv):
            print(json.dumps({"kernel": name, **c}))
        sys.exit(0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    asm = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else None
    if asm:
        args = [a for a in args if a != asm]
    src = args[0] if args and args[0].endswith((".hip", ".cpp")) else "voxelize_lists.hip"
    wanted = [a for a in args if a != src] or ["k_voxelize_listedILb0", "k_voxelize_queueILb0"]
    import json
    for name, c in counts(asm or assembly(src), wanted, "--hash" in sys.argv).items():
        print(json.dumps({"kernel": name, **c}))
