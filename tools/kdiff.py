#!/usr/bin/env python3
"""Kernel-by-kernel diff of a HIP source's gfx950 assembly against the same file at a git revision (a sibling of tools/kinfo.py).
   tools/kdiff.py [--mask] REV [zeekstd_amd/csrc/zk_decode.hip]
Both sides are compiled device side only with the Makefile's CXXFLAGS; REV's zeekstd_amd/csrc is unpacked into a temporary directory.
Per kernel, comment lines and trailing `;` comments are dropped, `__const.<mangled name>.` prefixes and the function number in local labels
become one token each, and the rest is compared as plain text:
   same                     nothing differs
   register numbers only    the texts are equal once every register number is masked (the metadata is equal too).  That is all it
                            says: a line whose operands changed places, or a renaming that is not consistent, looks the same
   DIFFERS                  the metadata of both sides and the unified diff
--mask prints the diff of the masked texts (v#, s#) instead: the hunks that are more than renumbering.  Every other differing line then
pairs with a line that differs from it in register numbers only, and their count is printed.
Exit status 1 if any kernel's vgpr_count, LDS, scratch or spill count differs, or a kernel exists on one side only."""
import difflib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "zeekstd_amd/csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")
GATED = ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def compile_start(src, out, flags):
    return subprocess.Popen([HIPCC, "--offload-arch=gfx950"] + flags + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.PIPE, text=True)


def kernels(path):
    """{mangled name: (metadata fields, normalised lines of the kernel's text)}"""
    text = open(path).read()
    found = {}
    for ent in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"\.?(\w+):\s+(\S+)", ent))
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(f["name"]), text, re.M | re.S).group(1)
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            ln = re.sub(r"__const\.\w+\.", "__const.K.", ln)
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        found[f["name"]] = (f, lines)
    return found


def masked(lines):
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", ln) for ln in lines]


def pretty(name):
    s = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", s).replace("void ", "")


def main():
    mask = "--mask" in sys.argv
    if mask:
        sys.argv.remove("--mask")
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    rel = os.path.relpath(os.path.abspath(sys.argv[2]), ROOT) if len(sys.argv) > 2 else CSRC + "/zk_decode.hip"
    with open(os.path.join(ROOT, CSRC, "Makefile")) as f:
        flags = re.search(r"^CXXFLAGS \?= (.*)$", f.read(), re.M).group(1).split()
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        jobs = [(rev, compile_start(os.path.join(d, rel), os.path.join(d, "old.s"), flags)),
                ("the working tree", compile_start(os.path.join(ROOT, rel), os.path.join(d, "new.s"), flags))]
        for side, j in jobs:
            err = j.communicate()[1]                         # (the compiler's warnings are dropped, its words on a failure are not)
            if j.returncode:
                sys.exit(f"kdiff: {rel} of {side} does not compile:\n{err}")
        old, new = kernels(os.path.join(d, "old.s")), kernels(os.path.join(d, "new.s"))
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    print(f"{rel}: {sha} (-) against the working tree (+), gfx950, {' '.join(flags)}")
    bad = nsame = 0
    for name in sorted(set(old) | set(new), key=pretty):
        if name not in old or name not in new:
            print(f"{pretty(name)}: only in {'the working tree' if name in new else sha}")
            bad += 1
            continue
        (fo, lo), (fn, ln) = old[name], new[name]
        meta_same = all(fo.get(k) == fn.get(k) for k in FIELDS)
        if lo == ln and meta_same:
            print(f"{pretty(name)}: same")
            nsame += 1
            continue
        if any(fo.get(k) != fn.get(k) for k in GATED):
            bad += 1
        renum = meta_same and masked(lo) == masked(ln)
        print(f"{pretty(name)}: {'register numbers only' if renum else 'DIFFERS'} ({len(lo)} -> {len(ln)} lines)")
        for side, f in (("-", fo), ("+", fn)):
            print("  " + side + " " + " ".join(f"{k} {f.get(k)}" for k in FIELDS))
        if mask and not renum:
            raw = sum(1 for h in difflib.unified_diff(lo, ln, lineterm="", n=0) if h[0] in "+-" and not h.startswith(("---", "+++")))
            lo, ln = masked(lo), masked(ln)
            left = sum(1 for h in difflib.unified_diff(lo, ln, lineterm="", n=0) if h[0] in "+-" and not h.startswith(("---", "+++")))
            print(f"  {raw} differing lines, {raw - left} of them in register numbers only; the others, register numbers masked:")
        if renum and mask:
            continue
        for h in difflib.unified_diff(lo, ln, lineterm="", n=2):
            if not h.startswith(("---", "+++")):
                print("  " + h)
    print(f"{nsame} of {len(set(old) | set(new))} kernels same; {bad} with different registers, LDS, scratch or spills")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
