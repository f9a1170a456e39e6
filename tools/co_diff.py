"""Compare the machine code of two sets of specialised-kernel code objects kernel by kernel (llvm-objdump -d, addresses
stripped - the pc-relative displacements of references to other symbols of the code object among them): `python tools/co_diff.py
DIR_A DIR_B` - which kernels exist on both sides and whether their instruction streams are identical.  (Stripping those displacements has a price: a call whose TARGET changed to another out-of-line function of the same code
object is not seen - the displacement is not resolved to a symbol name.  Where that matters, compare `llvm-objdump -t`'s
function symbols and their instruction counts too: the report lists both per symbol.)  Used to show that a refactoring or an `#ifdef`-gated experiment leaves the default kernels untouched.
With several code objects of one kernel in a directory (older builds), the NEWEST file wins."""
import os
import re
import subprocess
import sys

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(d):
    out = {}
    for f in sorted((f for f in os.listdir(d) if f.endswith(".co")), key=lambda f: os.path.getmtime(os.path.join(d, f))):
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", os.path.join(d, f)], capture_output=True, text=True).stdout
        name, body = None, []
        for line in txt.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                if name:
                    out[name] = (f, body)
                name, body = m.group(1), []
            elif name and line.strip():
                ins = re.sub(r"//.*$", "", line).strip()
                # `s_getpc_b64 s[a:b]; s_add_u32 sa, sa, <lit>; s_addc_u32 sb, sb, <lit>` forms the address of another symbol of the code
                # object (a function that was not inlined): the displacement is an address too - it moves when a kernel between the
                # two is added or removed, with no change to either
                pc = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", body[-1]) if body else None
                pc2 = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", body[-2]) if len(body) > 1 else None
                if pc and re.match(rf"s_add_u32 s{pc.group(1)}, s{pc.group(1)}, (0x[0-9a-f]+|-?\d+)$", ins):
                    ins = f"s_add_u32 s{pc.group(1)}, s{pc.group(1)}, <pc-relative>"
                elif pc2 and body[-1].endswith("<pc-relative>") and re.match(rf"s_addc_u32 s{pc2.group(2)}, s{pc2.group(2)}, (0x[0-9a-f]+|-?\d+)$", ins):
                    ins = f"s_addc_u32 s{pc2.group(2)}, s{pc2.group(2)}, <pc-relative>"
                body.append(ins)
        if name:
            out[name] = (f, body)
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    rc = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}: only in {'A' if k in a else 'B'}")
            continue
        same = a[k][1] == b[k][1]
        rc |= 0 if same else 1
        print(f"{k}: {'identical' if same else 'DIFFERENT'} ({len(a[k][1])} vs {len(b[k][1])} instructions; {a[k][0]} / {b[k][0]})")
    sys.exit(rc)
