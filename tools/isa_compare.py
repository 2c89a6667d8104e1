"""Compare the device code of two builds of csrc/ptycho_kernels.hip function by function (the acceptance test of a refactor:
the compiler's output does not change).

Build both trees with the Makefile's FLAGS plus ``--cuda-device-only -S -Rpass-analysis=kernel-resource-usage``, keeping the
assembly (``-o NAME.s``) and the remarks (``2> NAME.err``), then

    python tools/isa_compare.py LABEL parent.s parent.err branch.s branch.err [--table] [--float=NAME ...]

prints the number of functions, the number whose instruction stream is identical (comments stripped, the function number in
block labels normalised), every function that differs with its instruction counts, every function whose resource usage
(registers, spills, scratch, LDS, occupancy: what ``make usage`` prints) differs, and with ``--table`` the usage table itself.
``--float=NAME`` adds, for every function whose mangled name contains NAME, whether the ordered list of float32 arithmetic
instructions (add, sub, mul, fma, mac, plain and packed, whatever their encoding suffix) is the same in both builds, the
same for every mnemonic that names a float type at all, and the branch's count of each: the rounding of a kernel that is
allowed to differ elsewhere.
"""
import collections
import re
import shutil
import subprocess
import sys
import textwrap

LABEL = re.compile(r"\.L(func_begin|func_end|tmp)\d+")
ANY_FLOAT = re.compile(r"v_\w*f(16|32|64)\w*")   # conversions, compares, min / max, reciprocals ... as well
# plain and packed, with or without an encoding suffix (v_add_f32_e32, v_fma_f32, v_pk_mul_f32, v_fmac_f32_dpp ...)
FLOAT_OP = re.compile(r"v_(pk_)?(add|sub|subrev|mul|mul_legacy|fma|fmac|mac|mad|fmaak|fmamk|madak|madmk)_f32(_e32|_e64|_sdwa|_dpp)?\b")
USAGE_KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
              "LDS Size [bytes/block]")


def functions(path):
    """name -> list of normalised instruction lines"""
    out, name, body = {}, None, None
    with open(path, errors="replace") as f:
        for line in f:
            if name is None:
                m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
                if m:
                    name, body = m.group(1), []
                continue
            s = line.split(";", 1)[0].strip()
            if s.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            if not s or s == name + ":" or s.startswith(".p2align") or s.startswith(".globl") or s.startswith(".weak"):
                continue
            body.append(LABEL.sub(r".L\1", re.sub(r"\.LBB\d+_", ".LBB_", s)))
    return out


def usage(path):
    """name -> {key: value} from the kernel-resource-usage remarks"""
    out, cur = {}, None
    with open(path, errors="replace") as f:
        for line in f:
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\S+)", line)
            if m and cur is not None and m.group(1) in USAGE_KEYS:
                cur[m.group(1)] = m.group(2)
    return out


def demangle(names):
    if not names:
        return {}
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return dict(zip(names, names))
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    plain = r.stdout.splitlines() if r.returncode == 0 else names
    return dict(zip(names, plain))


def main():
    label, pa, pe, ba, be = sys.argv[1:6]
    table = "--table" in sys.argv[6:]
    floats = [a.split("=", 1)[1] for a in sys.argv[6:] if a.startswith("--float=")]
    differ_floats = False
    fp, fb = functions(pa), functions(ba)
    up, ub = usage(pe), usage(be)
    names = sorted(set(fp) | set(fb))
    differ = [n for n in names if fp.get(n) != fb.get(n)]
    udiff = [n for n in sorted(set(up) | set(ub)) if up.get(n) != ub.get(n)]
    nice = demangle(sorted(set(differ) | set(udiff)))
    print(f"== {label}: {len(fp)} functions in the parent, {len(fb)} in the branch, {len(names) - len(differ)} identical, "
          f"{sum(len(v) for v in fp.values())} / {sum(len(v) for v in fb.values())} instruction lines")
    for n in differ:
        a, b = fp.get(n), fb.get(n)
        print(f"   differs: {nice[n]}: {len(a) if a is not None else 'absent'} -> {len(b) if b is not None else 'absent'} lines")
    print(f"   resource usage: {len(up)} / {len(ub)} kernels, {len(udiff)} differ")
    for n in udiff:
        print(f"   usage differs: {nice[n]}: {up.get(n)} -> {ub.get(n)}")
    for want in floats:
        for n in (n for n in names if want in n and n in fp and n in fb):
            short = demangle([n])[n].split("(")[0]
            for what, pat in (("float32 arithmetic", FLOAT_OP), ("every float mnemonic", ANY_FLOAT)):
                a, b = ([s.split()[0] for s in f[n] if pat.match(s)] for f in (fp, fb))
                print(f"   {what} of {short}: {len(a)} -> {len(b)} instructions in order, "
                      f"{'identical' if a == b else 'DIFFERENT'}")
                differ_floats |= a != b
            mix = ", ".join(f"{v} {k}" for k, v in sorted(collections.Counter(b).items()))
            print(textwrap.fill("the branch's: " + mix, 124, initial_indent=" " * 6, subsequent_indent=" " * 8))
    if table:
        for who, u in (("parent", up), ("branch", ub)):
            print(f"   -- usage of the {who}: kernel | SGPRs | VGPRs | AGPRs | scratch | occupancy | SGPR spill | VGPR spill | LDS")
            for n in sorted(u):
                print("   " + n + " | " + " | ".join(u[n].get(k, "?") for k in USAGE_KEYS))
    return 1 if differ or udiff or differ_floats else 0


if __name__ == "__main__":
    sys.exit(main())
