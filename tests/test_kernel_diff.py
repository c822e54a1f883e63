"""tools/kernel_diff.py: the comparison of two builds' kernels, on tiny
synthetic instruction lists: identical, differs, added, removed, the padding behind a kernel's end
and --rename."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_diff  # noqa: E402

RES = (128, 0, 0)
BODY = ["s_load_dword s3, s[0:1], 0x28", "v_add_u32_e32 v1, s3, v0", "s_endpgm"]


def test_padding_behind_the_end_is_dropped():
    assert kernel_diff.strip_padding(BODY + ["s_nop 0"] * 5 + ["..."]) == BODY
    assert kernel_diff.strip_padding(BODY) == BODY
    # an s_nop that is code, not padding, stays: here nothing ends the kernel before it
    code = ["v_mov_b32_e32 v0, 0", "s_nop 1"]
    assert kernel_diff.strip_padding(code) == code
    inner = ["s_nop 0", "v_mov_b32_e32 v0, 0", "s_endpgm"]
    assert kernel_diff.strip_padding(inner + ["s_nop 0"]) == inner


def test_bare_names():
    assert kernel_diff.bare("k_a(unsigned int, void (*)(int))") == "k_a"
    assert kernel_diff.bare("void k_b<0, O1MapP>(O1Args, unsigned int*)") == "k_b<0, O1MapP>"
    assert kernel_diff.bare("_Zmangled") == "_Zmangled"


def test_identical_differs_added_removed():
    old = {"k_same(int)": (BODY + ["s_nop 0"] * 3, RES),
           "k_moved(int)": (BODY, RES),
           "k_regs(int)": (BODY, RES),
           "k_gone(int)": (BODY, RES)}
    new = {"k_same(int)": (BODY + ["s_nop 0"], RES),
           "k_moved(int)": (["s_load_dword s3, s[0:1], 0x30"] + BODY[1:], RES),
           "k_regs(int)": (BODY, (136, 0, 0)),
           "k_new(int)": (BODY, RES)}
    lines, count = kernel_diff.compare(old, new)
    assert count == {"identical": 1, "differs": 2, "added": 1, "removed": 1}
    by = {ln.split()[1]: ln for ln in lines[:-1]}
    assert by["k_same(int)"].startswith("identical") and "[3 instructions]" in by["k_same(int)"]
    assert "[3 -> 3 instructions, -1 +1 in 1 hunks]" in by["k_moved(int)"]
    assert "(128, 0, 0) -> (136, 0, 0)" in by["k_regs(int)"]
    assert by["k_new(int)"].startswith("added") and by["k_gone(int)"].startswith("removed")
    assert lines[-1] == "1 identical, 2 differs, 1 added, 1 removed"
    verbose, _ = kernel_diff.compare(old, new, verbose=True)
    assert "    -s_load_dword s3, s[0:1], 0x28" in verbose
    assert "    +s_load_dword s3, s[0:1], 0x30" in verbose


def test_rename_pairs_kernels():
    old = {"k_p(unsigned int, int*)": (BODY, RES), "void k_t<0>(Args)": (BODY, RES)}
    new = {"void k_p<true>(int*, unsigned int)": (BODY, RES),
           "void k_t<0, Map>(Args)": (BODY[:1] + ["v_mov_b32_e32 v2, 0"] + BODY[1:], RES)}
    _, count = kernel_diff.compare(old, new)
    assert count == {"identical": 0, "differs": 0, "added": 2, "removed": 2}
    lines, count = kernel_diff.compare(old, new, [("k_p", "k_p<true>"), ("k_t<0>", "k_t<0, Map>")])
    assert count == {"identical": 1, "differs": 1, "added": 0, "removed": 0}
    assert lines[0].startswith("identical void k_p<true>(int*, unsigned int)  (was k_p)")
    assert lines[1].startswith("differs   void k_t<0, Map>(Args)  (was k_t<0>)  [3 -> 4")
    # a rename whose target does not exist leaves both sides unpaired
    _, count = kernel_diff.compare(old, new, [("k_p", "k_q")])
    assert count == {"identical": 0, "differs": 0, "added": 2, "removed": 2}
