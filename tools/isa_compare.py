"""Compare the device code of two builds of csrc/ptycho_kernels.hip function by function (the acceptance test of a refactor:
the compiler's output does not change).

Build both trees with the Makefile's FLAGS plus ``--cuda-device-only -S -Rpass-analysis=kernel-resource-usage``, keeping the
assembly (``-o NAME.s``) and the remarks (``2> NAME.err``), then

    python tools/isa_compare.py LABEL parent.s parent.err branch.s branch.err [--table]

prints the number of functions, the number whose instruction stream is identical (comments stripped, the function number in
block labels normalised), every function that differs with its instruction counts, every function whose resource usage
(registers, spills, scratch, LDS, occupancy: what ``make usage`` prints) differs, and with ``--table`` the usage table itself.
"""
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.L(func_begin|func_end|tmp)\d+")
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
    if table:
        for who, u in (("parent", up), ("branch", ub)):
            print(f"   -- usage of the {who}: kernel | SGPRs | VGPRs | AGPRs | scratch | occupancy | SGPR spill | VGPR spill | LDS")
            for n in sorted(u):
                print("   " + n + " | " + " | ".join(u[n].get(k, "?") for k in USAGE_KEYS))
    return 1 if differ or udiff else 0


if __name__ == "__main__":
    sys.exit(main())
