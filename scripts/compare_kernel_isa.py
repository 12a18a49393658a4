"""Are the named kernels of two builds of libpf_hip.so the same instructions?  (no GPU needed)
usage: python scripts/compare_kernel_isa.py OLD.so NEW.so SUBSTRING [SUBSTRING ...]
Disassembles the gfx950 code objects of both libraries (llvm-objdump -d), keeps the kernels whose demangled name contains one
of the substrings, drops the address / encoding comment at the end of each line (the same instructions at another offset in
the library would differ there) and compares the listings kernel by kernel.  Exit status 1 if any kernel differs or is missing."""
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
    return out


def main(old, new, wanted):
    a, b = listings(old), listings(new)
    names = subprocess.run(["c++filt"], input="\n".join(a), capture_output=True, text=True).stdout.splitlines()
    bad = 0
    for sym, dem in zip(a, names):
        if not any(w in dem for w in wanted):
            continue
        if sym not in b:
            print(f"MISSING   {dem}")
            bad += 1
        elif a[sym] != b[sym]:
            print(f"DIFFERENT {dem}")
            sys.stdout.writelines(l + "\n" for l in list(difflib.unified_diff(a[sym], b[sym], lineterm="", n=1))[:40])
            bad += 1
        else:
            print(f"same      {dem}  ({len(a[sym])} lines)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
