"""Compare the gfx950 kernels of two builds of the library, kernel by kernel.

    python tools/kernel_diff.py [-v] OLD.so NEW.so

Every kernel of both libraries is disassembled (llvm-objdump -d of each code object, address and
encoding columns stripped; of a branch only its direction and of a pc-relative address only the
instruction are kept, since both distances move with any change elsewhere) and the two
instruction lists are compared.  One line per kernel: identical, added, removed, or differs with the instruction
counts of both sides and the number that changed.  The VGPR allocation, scratch and static LDS of
the kernel descriptors are compared too.  -v prints the differing hunks with a few lines of
context.  Exit status 0 whatever the result: the tool reports, the engineer judges (DESIGN.md
§9.9: a refactor may change straight-line setup and finish code of a kernel, never a loop body).
"""
import difflib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check  # noqa: E402

LLVM = isa_check.LLVM


def _resources(path):
    """{kernel: (VGPR allocation, scratch bytes per lane, static LDS bytes)} from the descriptors"""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-s", "-W", path], capture_output=True,
                         text=True, check=True).stdout
    data = open(path, "rb").read()
    secs = {}
    for line in out.splitlines():
        t = line.strip()
        m = re.match(r"\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)", t)
        if m:
            secs[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    res = {}
    for line in out.splitlines():
        p = line.split()
        if len(p) >= 8 and p[7].endswith(".kd") and p[6].isdigit():
            sa, so = secs[int(p[6])]
            at = so + int(p[1], 16) - sa
            lds, scratch = struct.unpack_from("<II", data, at)
            rsrc1 = struct.unpack_from("<I", data, at + 48)[0]
            res[p[7][:-3]] = (((rsrc1 & 63) + 1) * 8, scratch, lds)
    return res


def kernels(lib):
    """{kernel: ([instruction text], resources)} of every gfx950 kernel in lib"""
    out = {}
    for blob in isa_check.code_objects(lib):
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "co")
            open(path, "wb").write(blob)
            res = _resources(path)
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", path],
                                 capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1) if m.group(1) in res else None
                if cur:
                    out[cur] = ([], res[cur])
                continue
            text = line.split("//")[0].strip()
            if cur and text:
                # the literal added to s_getpc_b64's result (a far branch, the address of a
                # global) moves with any change of size anywhere in the code object: keep the
                # instruction, drop the distance
                code = out[cur][0]
                if code and code[-1].startswith("s_getpc_b64") and text.startswith("s_add_u32"):
                    text = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", text)
                # likewise a branch's distance (in dwords, 16-bit two's complement), which
                # changes when anything between the branch and its target does: its direction stays
                m = re.fullmatch(r"(s_c?branch\w*) (\d+)", text)
                if m:
                    text = f"{m.group(1)} <{'back' if int(m.group(2)) >= 0x8000 else 'forward'}>"
                code.append(text)
    return out


def demangle(names):
    """names -> readable names, where a demangler is installed"""
    tool = next((t for t in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt")) if t and
                 os.path.exists(t)), None)
    nice = []
    if tool:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        nice = r.stdout.splitlines() if r.returncode == 0 else []
    return dict(zip(names, nice)) if len(nice) == len(names) else {n: n for n in names}


def main(argv):
    verbose = "-v" in argv
    libs = [a for a in argv if a != "-v"]
    if len(libs) != 2:
        print(__doc__)
        return 0
    old, new = kernels(libs[0]), kernels(libs[1])
    names = sorted(set(old) | set(new))
    nice = demangle(names)
    count = {"identical": 0, "differs": 0, "added": 0, "removed": 0}
    for k in names:
        if k not in old or k not in new:
            what = "added" if k not in old else "removed"
            count[what] += 1
            print(f"{what:9s} {nice[k]}")
            continue
        (a, ra), (b, rb) = old[k], new[k]
        res = "" if ra == rb else f"  (VGPRs, scratch, LDS) {ra} -> {rb}"
        if a == b and ra == rb:
            count["identical"] += 1
            print(f"identical {nice[k]}  [{len(a)} instructions]")
            continue
        count["differs"] += 1
        sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
        ops = [o for o in sm.get_opcodes() if o[0] != "equal"]
        gone = sum(o[2] - o[1] for o in ops)
        come = sum(o[4] - o[3] for o in ops)
        print(f"differs   {nice[k]}  [{len(a)} -> {len(b)} instructions, -{gone} +{come} in "
              f"{len(ops)} hunks]{res}")
        if verbose:
            for line in difflib.unified_diff(a, b, "old", "new", n=3, lineterm=""):
                print("    " + line)
    print(", ".join(f"{v} {k}" for k, v in count.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
