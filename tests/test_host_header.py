"""The host side of the library keeps its types and its cross-unit prototypes in one internal
header: rc_ctx and rc_model are defined in csrc/rc_host.h and nowhere else, no
unit reaches into them through a shim, and no .hip or .inc file declares a function of another
unit by hand.  (CPU: source text only.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "range_coder_rust_amd", "csrc")

# the accessors that stood in for the fields while the types were private to rc_kernels.hip
SHIMS = ("rc_ctx_stream_", "rc_ctx_knobs_", "rc_model_describe_", "rc_model_is_set_",
         "rc_model_is_wide_", "rc_model_is_order1_", "rc_model_wide_row_",
         "rc_model_order1_rows_", "rc_model_order1_period_", "rc_model_order1_lag_")


def _sources(suffixes=(".hip", ".inc", ".h", ".cpp")):
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(suffixes):
            with open(os.path.join(CSRC, f)) as fh:
                out[f] = fh.read()
    return out


def _code(text):
    """The text without comments, preprocessor lines (continuations included) and the contents of
    string literals; extern "C" survives as one word."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"(?m)^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text)
    text = text.replace('extern "C"', "extern_C")
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"'(?:\\.|[^'\\\n])'", "' '", text)


def _file_scope_statements(text):
    """The statements at file scope, one string each (newlines and all).  extern "C" { and
    namespace ... { do not leave file scope; every other braced block (a function body, a struct,
    an initializer) is cut down to {} and, when nothing but a ; can follow it, ends its
    statement."""
    code = _code(text)
    out, cur, stack, par = [], [], [], 0
    for i, ch in enumerate(code):
        inner = any(not t for t in stack)  # inside a block that is not transparent
        if ch == "{":
            head = "".join(cur) if not inner else ""
            transparent = not inner and par == 0 and re.search(
                r"(?:\bextern_C|\bnamespace(?:\s+\w+)?)\s*$", head) is not None
            stack.append(transparent)
            if transparent:
                cur = []
            elif not inner:
                cur.append("{")
        elif ch == "}":
            transparent = stack.pop() if stack else True
            if not transparent and not any(not t for t in stack):
                cur.append("}")
                if par == 0 and not re.match(r"\s*;", code[i + 1:]):
                    out.append("".join(cur))
                    cur = []
        elif not inner:
            par += (ch == "(") - (ch == ")")
            if ch == ";" and par == 0:
                out.append("".join(cur))
                cur = []
            else:
                cur.append(ch)
    return out


# a declaration's head: a type, then the name, then the parameter list (a statement with an =
# or a ( before the name is an initializer or a call; __attribute__ and its like are no names)
_PROTO = re.compile(r"^[^=(]*?[\w>\*&]\s+[\*&]*\b(?!__)(\w+_|set_allow_lds)\s*\(", re.S)


def _prototypes(text):
    return [m.group(1) for m in (_PROTO.match(s) for s in _file_scope_statements(text))
            if m and "{" not in m.string]


def test_the_prototype_finder_copes_with_several_lines_and_skips_the_rest():
    sample = '''
    // void in_a_comment_(int);
    #define MACRO_(x) \\
      void in_a_macro_(x);
    extern "C" {
    rc_status rc_over_lines_(rc_ctx* ctx,
                             hipStream_t* s,   // the stream
                             int* device);
    }
    namespace {
    hipError_t set_allow_lds(const void* kernel);
    static const u32*
    two_line_head_(int a);
    struct S { void member_(int); };
    void defined_(int a) { called_(a); other_(a, (int)a); }
    u32 g_value = initialised_(3);
    typedef __attribute__((address_space(3))) u32 l_u32;
    }  // namespace
    template <int N> void plain_name(int);
    '''
    assert _prototypes(sample) == ["rc_over_lines_", "set_allow_lds", "two_line_head_"]


def test_the_context_and_the_model_are_defined_once_in_rc_host_h():
    for what in ("struct rc_ctx {", "struct rc_model {"):
        where = [f for f, text in _sources().items() for _ in range(text.count(what))]
        assert where == ["rc_host.h"], (what, where)


def test_no_shim_is_left():
    found = [(f, name) for f, text in _sources().items() for name in SHIMS if name in text]
    assert not found, found


def test_no_unit_forward_declares_the_types():
    found = [(f, m.group(0)) for f, text in _sources((".hip", ".inc")).items()
             for m in re.finditer(r"\bstruct\s+rc_(?:ctx|model)\s*;", _code(text))]
    assert not found, found


def test_no_unit_writes_a_prototype_of_anothers_function():
    found = [(f, name) for f, text in _sources((".hip", ".inc")).items()
             for name in _prototypes(text)]
    assert not found, found
