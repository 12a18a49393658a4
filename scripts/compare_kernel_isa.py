"""Are the named kernels of two builds of libpf_hip.so the same instructions?  (no GPU needed)
usage: python scripts/compare_kernel_isa.py OLD.so NEW.so PATTERN [PATTERN ...]
Disassembles the gfx950 code objects of both libraries (llvm-objdump -d), drops the address / encoding comment at the end of each
line (the same instructions at another offset in the library would differ there) and the trailing run of padding lines
behind a kernel's final instruction (s_nop 0, s_code_end, objdump's "..."; it depends on what was placed next) and compares the listings kernel by kernel.
PATTERN is either
  SUBSTRING  every kernel of OLD.so whose demangled name contains it, against the kernel of the same mangled symbol in NEW.so
  OLD=NEW    a renamed kernel: the one kernel of OLD.so whose demangled name contains OLD against the one of NEW.so whose name
             contains NEW.  A side that matches no kernel or more than one is an error, so '<3>' is never compared with '<5>'.
Exit status 1 if any kernel differs, is missing or a renaming pattern is not unique."""
import difflib
import importlib.util
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(HERE, "kernel_resources.py"))
kr = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kr)

PADDING = ("s_nop 0", "s_code_end", "...")


def listings(lib):
    """{mangled symbol: [instruction lines without the trailing comment]} over every gfx950 code object of the library"""
    out = {}
    for co in kr.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in text.splitlines():
            if line.endswith(">:"):
                cur = line.split("<")[1][:-2]
                out[cur] = []
            elif cur is not None and line.strip():
                out[cur].append(line.split("//")[0].strip())
    for ins in out.values():  # a trailing run of padding behind the final instruction is filler up to the next symbol or the end of the section
        while ins and ins[-1] in PADDING:
            ins.pop()
    return out


def demangled(syms):
    return dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()))


def pairs(da, db, wanted):
    """[(name in the old library, old symbol, new symbol or None)] for the patterns; raises SystemExit on an ambiguous OLD=NEW"""
    out = []
    for w in wanted:
        if "=" in w:
            old, new = w.split("=", 1)
            ma, mb = [s for s, d in da.items() if old in d], [s for s, d in db.items() if new in d]
            if len(ma) != 1 or len(mb) != 1:
                sys.exit(f"{w}: '{old}' matches {len(ma)} kernels of the old library and '{new}' {len(mb)} of the new one; each must match one\n  "
                         + "\n  ".join([da[s] for s in ma] + [db[s] for s in mb]))
            out.append((f"{da[ma[0]]}  ->  {db[mb[0]]}", ma[0], mb[0]))
        else:
            out += [(d, s, s if s in db else None) for s, d in da.items() if w in d]
    return out


def main(old, new, wanted):
    a, b = listings(old), listings(new)
    bad = 0
    for dem, sa, sb in pairs(demangled(list(a)), demangled(list(b)), wanted):
        if sb is None:
            print(f"MISSING   {dem}")
            bad += 1
        elif a[sa] != b[sb]:
            print(f"DIFFERENT {dem}")
            sys.stdout.writelines(l + "\n" for l in list(difflib.unified_diff(a[sa], b[sb], lineterm="", n=1))[:40])
            bad += 1
        else:
            print(f"same      {dem}  ({len(a[sa])} lines)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
