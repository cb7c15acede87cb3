"""Prove that a refactor left the generated gfx950 device code alone.

    python tools/kernel_isa_diff.py [--base REV] [--jobs N] [--log FILE]

Compiles every csrc/*.hip of REV (default HEAD, taken with `git archive`) and of the working tree with _capi.HIPCC_FLAGS plus
-save-temps, cuts the gfx950 assembly into functions (label .. .Lfunc_end) and kernel descriptors (.amdhsa_kernel ..
.end_amdhsa_kernel) and compares them by mangled name.  Comments, .loc / .file lines and the numbering of local labels
(.LBB<n>_, .Ltmp<n>, .Lfunc_end<n>) do not count.  A name may be emitted by several translation units (helpers in
anonymous namespaces): its set of distinct bodies must be the same on both sides.  One line per function; exit status 1
when a function changed, vanished or appeared.  Needs hipcc only: no GPU, no network.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparse_rx import _capi  # noqa: E402

CSRC_REL = os.path.relpath(_capi.CSRC_DIR, ROOT)
INC_REL = os.path.relpath(_capi.INCLUDE_DIR, ROOT)


def compile_tree(tree, out, jobs):
    """hipcc -save-temps of every .hip under tree/CSRC_REL, one working directory per source -> {unit: path of its .s}"""
    hipcc = _capi.shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc, inc = os.path.join(tree, CSRC_REL), os.path.join(tree, INC_REL)

    def one(src):
        unit = os.path.basename(src)
        wd = os.path.join(out, unit)
        os.makedirs(wd)
        subprocess.run([hipcc, *_capi.HIPCC_FLAGS, "-save-temps", f"-I{inc}", f"-I{csrc}", "-c", "-o", "unit.o", src], cwd=wd, check=True,
                       stderr=subprocess.DEVNULL)  # -save-temps warns about every unused argument
        (asm,) = glob.glob(os.path.join(wd, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))
        return unit, asm

    with ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, sorted(glob.glob(os.path.join(csrc, "*.hip")))))


def functions(asm_path):
    """{mangled name: normalised text of the body + the kernel descriptor} of one gfx950 .s file"""
    body, desc, cur, name = {}, {}, None, None
    for raw in open(asm_path):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip() or re.match(r"\s*\.(loc|file)\s", line):
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
        elif name and line == name + ":":
            cur, name = body.setdefault(line[:-1], []), None
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"\s*\.amdhsa_kernel\s", line):
            cur = desc.setdefault(line.split()[1], [])
        elif re.match(r"\s*\.end_amdhsa_kernel", line):
            cur = None
        elif cur is not None:
            cur.append(line)
    assert set(desc) <= set(body), "descriptor without a function body"
    return {n: "\n".join(b) + "\n--descriptor--\n" + "\n".join(desc.get(n, [])) for n, b in body.items()}


def collect(units):
    """{name: {text: [units that emit it]}}"""
    out = {}
    for unit, asm in sorted(units.items()):
        for n, text in functions(asm).items():
            out.setdefault(n, {}).setdefault(text, []).append(unit)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--log", default=None, help="also write the report to this file")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base_tree = os.path.join(tmp, "base_tree")
        os.makedirs(base_tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC_REL, INC_REL], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", base_tree], input=tar, check=True)
        old = collect(compile_tree(base_tree, os.path.join(tmp, "base_out"), a.jobs))
        new = collect(compile_tree(ROOT, os.path.join(tmp, "new_out"), a.jobs))
    where = lambda side: ",".join(sorted(u for us in side.values() for u in us))
    lines, bad = [], 0
    for n in sorted(set(old) | set(new)):
        o, w = old.get(n, {}), new.get(n, {})
        status = "identical" if set(o) == set(w) else "ADDED" if not o else "MISSING" if not w else "DIFFERENT"
        bad += status != "identical"
        kind = "kernel  " if any(not t.endswith("--descriptor--\n") for t in list(o) + list(w)) else "function"
        lines.append(f"{status:9s} {kind} {n}  [{where(o) or '-'} -> {where(w) or '-'}]")
    base_rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.base], check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    lines.append(f"# base {base_rev}: {len(old)} functions, working tree: {len(new)} functions, not identical: {bad}")
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if a.log:
        with open(a.log, "w") as fh:
            fh.write(report)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
