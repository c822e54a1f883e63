"""Compare the gfx950 kernels of two builds of the library, kernel by kernel.

    python tools/kernel_diff.py [-v] [--rename OLD=NEW]... OLD.so NEW.so

Every kernel of both libraries is disassembled (llvm-objdump -d of each code object, address and
encoding columns stripped; of a branch only its direction and of a pc-relative address only the
instruction are kept, since both distances move with any change elsewhere; the s_nop padding
behind a kernel's last s_endpgm is dropped, since it follows the size of the kernel's neighbours)
and the two instruction lists are compared.  One line per kernel: identical, added, removed, or
differs with the instruction counts of both sides and the number that changed.  --rename pairs
kernel OLD of the old library with kernel NEW of the new one (demangled names without return type
and parameter list, e.g. 'k_decode_o1p<0>=k_decode_order1<0, O1MapP>'), so a renamed kernel is
compared, not reported as one removed and one added.  The VGPR allocation, scratch and static LDS of
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




def strip_padding(code):
    """code without the padding behind its last s_endpgm (s_nop, or zero bytes, which the
    disassembler prints as "..."): the assembler pads a kernel up to the alignment of the next
    one, so the padding follows the sizes of the kernel's neighbours"""
    end = len(code)
    while end and (code[end - 1].startswith("s_nop") or code[end - 1] == "..."):
        end -= 1
    return code[:end] if end and code[end - 1].startswith("s_endpgm") else code


def bare(name):
    """a demangled kernel name without its return type and parameter list: what --rename names"""
    name = name[5:] if name.startswith("void ") else name
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def compare(old, new, renames=(), verbose=False):
    """old, new: {readable kernel name: ([instruction text], resources)}; renames: (OLD, NEW)
    pairs of bare names, a kernel OLD of `old` being compared with the kernel NEW of `new`.
    Returns (report lines, {"identical", "differs", "added", "removed": counts})."""
    renames = dict(renames)
    by_bare = {bare(k): k for k in new}
    pairs, taken = [], set()
    for k in sorted(old):
        to = by_bare.get(renames.get(bare(k))) if bare(k) in renames else (k if k in new else None)
        pairs.append((k, to))
        taken.add(to)
    pairs += [(None, k) for k in sorted(new) if k not in taken]
    lines, count = [], {"identical": 0, "differs": 0, "added": 0, "removed": 0}
    for ko, kn in sorted(pairs, key=lambda p: p[1] or p[0]):
        if ko is None or kn is None:
            what = "added" if ko is None else "removed"
            count[what] += 1
            lines.append(f"{what:9s} {kn or ko}")
            continue
        title = kn if ko == kn else f"{kn}  (was {bare(ko)})"
        (a, ra), (b, rb) = old[ko], new[kn]
        a, b = strip_padding(a), strip_padding(b)
        res = "" if ra == rb else f"  (VGPRs, scratch, LDS) {ra} -> {rb}"
        if a == b and ra == rb:
            count["identical"] += 1
            lines.append(f"identical {title}  [{len(a)} instructions]")
            continue
        count["differs"] += 1
        sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
        ops = [o for o in sm.get_opcodes() if o[0] != "equal"]
        gone = sum(o[2] - o[1] for o in ops)
        come = sum(o[4] - o[3] for o in ops)
        lines.append(f"differs   {title}  [{len(a)} -> {len(b)} instructions, -{gone} +{come} in "
                     f"{len(ops)} hunks]{res}")
        if verbose:
            lines += ["    " + line for line in difflib.unified_diff(a, b, "old", "new", n=3,
                                                                      lineterm="")]
    lines.append(", ".join(f"{v} {k}" for k, v in count.items()))
    return lines, count


def main(argv):
    verbose, renames, libs = False, [], []
    args = iter(argv)
    for a in args:
        if a == "-v":
            verbose = True
        elif a == "--rename" or a.startswith("--rename="):
            spec = a[9:] if a.startswith("--rename=") else next(args, "")
            if "=" not in spec:
                print(__doc__)
                return 0
            renames.append(tuple(spec.split("=", 1)))
        else:
            libs.append(a)
    if len(libs) != 2:
        print(__doc__)
        return 0
    both = []
    for lib in libs:
        ks = kernels(lib)
        nice = demangle(sorted(ks))
        both.append({nice[k]: v for k, v in ks.items()})
    print("\n".join(compare(both[0], both[1], renames, verbose)[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
