"""Is the device code of this tree the same as another tree's?  (no GPU needed)

    python profiles/isa_identical.py <other-tree> [-DNAME[=value] ...]

Compiles every csrc/*.hip of this tree and of the other one (a checkout of another commit) to gfx950 assembly with this tree's
compile command (brdf_nerf_amd/build.py compile_command; the -D arguments go to both sides), drops the lines that carry the
per-file __hip_cuid_<hash> symbol and prints, per file, `identical` or the first kernel whose code differs.  Exit status 1 on
any difference.  A refactor that moves no instruction shows it here: source hashes differ, code objects do not."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from brdf_nerf_amd import build as B  # noqa: E402


def assembly(src, defs, out):
    """the assembly's lines, or (a string) the compiler's first error line"""
    r = subprocess.run(B.compile_command(src, out, defs, asm=True), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        return next((l for l in r.stderr.splitlines() if "error" in l), "hipcc exit status %d" % r.returncode)
    return [l for l in open(out) if "__hip_cuid_" not in l]


def main():
    other = os.path.join(os.path.abspath(sys.argv[1]), os.path.relpath(B.CSRC, ROOT))
    defs = [a[2:] for a in sys.argv[2:] if a.startswith("-D")]
    names = sorted(set(f for d in (B.CSRC, other) for f in os.listdir(d) if f.endswith(".hip")))
    bad = 0
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        jobs = {(d, f): ex.submit(assembly, os.path.join(d, f), defs, os.path.join(td, ("this_" if d == B.CSRC else "other_") + f + ".s"))
                for f in names for d in (B.CSRC, other) if os.path.exists(os.path.join(d, f))}
        for f in names:
            if (B.CSRC, f) not in jobs or (other, f) not in jobs:
                print(f"{f}: only in {'this' if (B.CSRC, f) in jobs else 'the other'} tree")
                bad = 1
                continue
            a, b = jobs[(B.CSRC, f)].result(), jobs[(other, f)].result()
            if isinstance(a, str) or isinstance(b, str):
                for side, r in (("this", a), ("the other", b)):
                    if isinstance(r, str):
                        print(f"{f}: does not compile in {side} tree: {r}")
                bad = 1
                continue
            if a == b:
                print(f"{f}: identical ({len(a)} lines)")
                continue
            bad = 1
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            kernel = next((m.group(1) for l in reversed(a[:i + 1]) for m in [re.match(r"^(\w+):", l)] if m), "(before the first symbol)")
            print(f"{f}: DIFFERS first at line {i + 1}, in {kernel}")
    sys.exit(bad)


if __name__ == "__main__":
    main()
