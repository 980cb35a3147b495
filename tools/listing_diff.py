"""Compare two device listings of one translation unit kernel by kernel (hipcc -S --cuda-device-only with build_hip's flags).

Per kernel: the instruction text with comments, directives and labels stripped and block labels renumbered in order of appearance
(so that a kernel that merely moved inside the unit compares equal), the count of every opcode (without the assembler's encoding
suffix: _e32 / _e64 / _dpp / _sdwa name one opcode), and the VGPR count and scratch size of its .amdhsa_kernel block.  Verdict
per kernel:
  identical          the same instruction text
  fp opcodes equal   the text differs, every opcode whose name contains one of --fp (default _f16,_f32,_f64) occurs equally often
  FP OPCODES DIFFER  otherwise (the differing opcodes follow)
and "VGPRS UP" / "SCRATCH UP" where the second listing needs more than the first.  Exit status 1 if a kernel named by --moved
(a substring of the demangled name; repeatable) is not at least "fp opcodes equal" or needs more registers or scratch, if any
other kernel is not "identical", or if the two listings do not hold the same kernels.
usage: python tools/listing_diff.py PARENT.s CHANGE.s [--moved SUBSTRING]... [--fp _f32,...]"""
import argparse
import collections
import re
import shutil
import subprocess
import sys

ENCODING = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")   # the assembler's encoding suffix: the same opcode either way


def kernels(path):
    """mangled name -> dict(text=[instructions], vgprs, scratch) for every .amdhsa_kernel of the listing."""
    lines = open(path).read().split("\n")
    meta, name = {}, None
    for ln in lines:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            name = s.split()[1]
            meta[name] = {}
        elif s == ".end_amdhsa_kernel":
            name = None
        elif name and s.startswith(".amdhsa_"):
            k, _, v = s.partition(" ")
            meta[name][k] = v.strip()
    out, cur = {}, None
    for ln in lines:
        s = ln.split(";")[0].strip()
        if s.endswith(":") and s[:-1] in meta:
            cur = out.setdefault(s[:-1], [])
            continue
        if cur is None or not s:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        elif not s.startswith(".") and not s.endswith(":"):
            cur.append(re.sub(r"\s+", " ", s))
    res = {}
    for name, text in out.items():
        labels = {}
        text = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), t) for t in text]
        res[name] = dict(text=text, vgprs=int(meta[name].get(".amdhsa_next_free_vgpr", "0")),
                         scratch=int(meta[name].get(".amdhsa_private_segment_fixed_size", "0")))
    return res


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    got = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("--moved", action="append", default=[])
    ap.add_argument("--fp", default="_f16,_f32,_f64")
    args = ap.parse_args()
    fp = args.fp.split(",")
    a, b = kernels(args.parent), kernels(args.change)
    bad = sorted(set(a) ^ set(b))
    for n in bad:
        print(f"ONLY IN {'parent' if n in a else 'change'}: {n}")
    names = sorted(set(a) & set(b))
    nice = demangle(names)
    nice = {n: re.sub(r"\(anonymous namespace\)::|^void ", "", v).split("(")[0] for n, v in nice.items()}
    print(f"# {'kernel':70s} {'instr p/c':>13s} {'vgprs p/c':>9s} {'scratch p/c':>11s}  verdict")
    fail = bool(bad)
    for n in sorted(names, key=lambda n: nice[n]):
        ka, kb = a[n], b[n]
        moved = any(m in nice[n] for m in args.moved)
        if ka["text"] == kb["text"]:
            verdict = "identical"
        else:
            ca = collections.Counter(ENCODING.sub("", t.split()[0]) for t in ka["text"])
            cb = collections.Counter(ENCODING.sub("", t.split()[0]) for t in kb["text"])
            diff = {op: (ca[op], cb[op]) for op in set(ca) | set(cb) if ca[op] != cb[op] and any(f in op for f in fp)}
            verdict = "fp opcodes equal" if not diff else "FP OPCODES DIFFER " + " ".join(f"{op} {x}/{y}" for op, (x, y) in sorted(diff.items()))
            fail = fail or bool(diff) or not moved
        if kb["vgprs"] > ka["vgprs"]:
            verdict, fail = verdict + "  VGPRS UP", True
        if kb["scratch"] > ka["scratch"]:
            verdict, fail = verdict + "  SCRATCH UP", True
        print(f"{('* ' if moved else '  ') + nice[n]:72s} {len(ka['text']):6d}/{len(kb['text']):<6d} {ka['vgprs']:4d}/{kb['vgprs']:<4d} "
              f"{ka['scratch']:5d}/{kb['scratch']:<5d}  {verdict}")
    print(f"# {len(names)} kernels, * = named by --moved; {'FAILED' if fail else 'ok'}")
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())
