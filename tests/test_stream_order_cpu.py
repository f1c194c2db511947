"""CPU: the table behind tests/test_stream_order_gpu.py is complete.  Every function of include/pnp_hip.h that takes a `void*
stream` is gated by a case or excluded as an alias of a gated sibling; every MAY_BLOCK entry quotes the header; and every Python
wrapper that forwards to such a function hands it the current stream."""
import ast
import os
import re

import pytest

pytest.importorskip("torch")

import _stream_gate as G          # noqa: E402
import test_stream_order_gpu as T          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pnp_hip.h")
WRAPPERS = [os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", f) for f in ("hip.py", "crf.py")]


def _stream_functions():
    """Names of the declared functions whose last parameter is `void* stream`, as tests/test_cabi_cpu.py reads the header."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\b(pnp_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        if re.search(r"void\s*\*\s*stream\s*$", params.strip()):
            out.append(name)
    return sorted(set(out))


def _covered():
    return sorted({f for covers, _, _ in T.CASES.values() for f in covers})


def test_header_parse_finds_the_stream_functions():
    names = _stream_functions()
    assert len(names) >= 60, names
    for must in ("pnp_vit_forward", "pnp_op_gemm_x3", "pnp_crf_backward_terms", "pnp_png_encode", "pnp_jpeg_decode_scans", "pnp_op_cls_rows"):
        assert must in names
    for never in ("pnp_create", "pnp_crf_set_compat", "pnp_op_gemm_plan", "pnp_get_buffer"):
        assert never not in names


def test_every_stream_function_is_gated_or_an_excluded_alias():
    names, covered = set(_stream_functions()), set(_covered())
    assert covered <= names, sorted(covered - names)
    assert set(T.EXCLUDED) <= names, sorted(set(T.EXCLUDED) - names)
    assert not covered & set(T.EXCLUDED), sorted(covered & set(T.EXCLUDED))
    missing = sorted(names - covered - set(T.EXCLUDED))
    assert not missing, f"no case of tests/test_stream_order_gpu.py gates {missing}"
    for name, reason in T.EXCLUDED.items():
        assert reason and "\n" not in reason, name
        siblings = set(re.findall(r"pnp_[a-z_0-9]+", reason))
        assert siblings and siblings <= covered, f"{name} is excluded as an alias of {sorted(siblings)}: not gated"


def test_cases_that_may_hold_the_host_name_a_may_block_entry_point():
    for name, (covers, _, may_block) in T.CASES.items():
        assert covers, name
        if may_block:
            assert any(f in G.MAY_BLOCK for f in covers), name


def _comments_about(text, name):
    """The comment blocks of the header that speak of `name`: those that name it, and those between the previous function
    declaration and its own (its descriptor structs and their comments sit there).  Flattened: the ` * ` line starts and the
    line breaks of a block become single blanks."""
    blank = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    decls = [m.start() for m in re.finditer(r"\bpnp_[a-z_0-9]+\s*\(", blank)]
    mine = re.search(r"\b" + name + r"\s*\(", blank).start()
    prev = max([d for d in decls if d < mine], default=0)
    out = []
    for m in re.finditer(r"/\*.*?\*/", text, flags=re.S):
        flat = re.sub(r"\s+", " ", re.sub(r"\n\s*\*\s?", " ", m.group(0)))
        if re.search(r"\b" + name + r"\b", flat) or prev < m.start() < mine:
            out.append(flat)
    return out


def test_may_block_entries_quote_the_header():
    """Every entry takes a stream (a case can reach it), and its quote stands in a comment of the header that is about that
    function -- one that names it or the one in front of its declaration -- and says that the call synchronises."""
    text = open(HEADER).read()
    streams = set(_stream_functions())
    for name, quote in G.MAY_BLOCK.items():
        assert name in streams, f"{name} takes no stream: no gated call can reach it"
        assert re.search(r"[Ss]ynchroni[sz]e", quote), f"{name}: {quote!r} does not say that the call synchronises"
        want = re.sub(r"\s+", " ", quote)
        assert len(quote) >= 20 and any(want in c for c in _comments_about(text, name)), (
            f"{name}: no comment of include/pnp_hip.h about it says {quote!r}")
    covered = {f for covers, _, may_block in T.CASES.values() if may_block for f in covers}
    assert set(G.MAY_BLOCK) <= covered, sorted(set(G.MAY_BLOCK) - covered)     # every entry is met by a case that lets it hold the host


def _is_current_stream(node):
    """_stream() | hip._stream() | torch.cuda.current_stream().cuda_stream"""
    src = ast.unparse(node)
    return src in ("_stream()", "hip._stream()", "torch.cuda.current_stream().cuda_stream")


def test_python_wrappers_pass_the_current_stream():
    """Every call of a stream function in pnp_ovss/hip.py and pnp_ovss/crf.py ends in the current stream.  The one exception:
    the size queries of the encoders (first argument None: d_ws = NULL only computes *ws_need, nothing is launched)."""
    names = set(_stream_functions())
    seen = set()
    for path in WRAPPERS:
        for node in ast.walk(ast.parse(open(path).read())):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names):
                continue
            where = f"{os.path.basename(path)}:{node.lineno} {node.func.attr}"
            assert node.args and not node.keywords, where
            first, last = node.args[0], node.args[-1]
            if isinstance(last, ast.Constant) and last.value is None and isinstance(first, ast.Constant) and first.value is None:
                assert node.func.attr in ("pnp_jpeg_encode", "pnp_png_encode"), where
                continue
            assert not isinstance(last, ast.Constant), f"{where}: a literal {last.value!r} in the stream position"
            assert _is_current_stream(last), f"{where}: the stream argument is {ast.unparse(last)}"
            seen.add(node.func.attr)
    # what the wrappers do not forward to at all is reached through ctypes by the tests alone
    assert len(seen) >= 30, sorted(seen)
