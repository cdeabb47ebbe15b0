"""CPU tests (no GPU): the warp-ctc C API of include/ctc.h -- compute_ctc_loss, get_workspace_size, ctcGetStatusString -- is exported by
libctc_crf_hip.so with C linkage, its header compiles as C, and get_workspace_size (host-only) checks its arguments and sizes monotonically."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

API = ("compute_ctc_loss", "get_workspace_size", "ctcGetStatusString")
INVALID_VALUE = 2


class Opt(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("blank_label", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    import ctc_crf
    lib = ctypes.CDLL(ctc_crf._C.LIB_PATH)
    lib.ctcGetStatusString.argtypes = [ctypes.c_int]
    lib.ctcGetStatusString.restype = ctypes.c_char_p
    lib.get_workspace_size.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, Opt,
                                       ctypes.POINTER(ctypes.c_size_t)]
    lib.get_workspace_size.restype = ctypes.c_int
    return lib


def _ws(lib, label_lengths, input_lengths, V, B=None, blank=0):
    ll = (ctypes.c_int * max(1, len(label_lengths)))(*label_lengths)
    il = (ctypes.c_int * max(1, len(input_lengths)))(*input_lengths)
    size = ctypes.c_size_t(0)
    st = lib.get_workspace_size(ll, il, V, len(label_lengths) if B is None else B, Opt(None, blank), ctypes.byref(size))
    return st, size.value


def test_symbols_exported_with_c_linkage(lib):
    import ctc_crf
    for s in API:
        assert hasattr(lib, s), s
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", ctc_crf._C.LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in API:
        assert s in syms, f"{s} is not a plain (unmangled) dynamic symbol"


def test_status_strings(lib):
    txt = [lib.ctcGetStatusString(i) for i in range(5)]
    assert all(t for t in txt) and len(set(txt)) == 5, txt


def test_workspace_size_rejects_bad_arguments(lib):
    assert _ws(lib, [3, 2], [10, 8], 0)[0] == INVALID_VALUE            # alphabet_size <= 0
    assert _ws(lib, [3, 2], [10, 8], -4)[0] == INVALID_VALUE
    assert _ws(lib, [3, 2], [10, 8], 72, B=0)[0] == INVALID_VALUE      # minibatch <= 0
    assert _ws(lib, [3, -1], [10, 8], 72)[0] == INVALID_VALUE          # negative label length
    assert _ws(lib, [3, 2], [10, -8], 72)[0] == INVALID_VALUE          # negative input length
    assert _ws(lib, [2048, 2], [5000, 8], 72)[0] == INVALID_VALUE      # label length over the build's limit
    st, n = _ws(lib, [2047, 2], [5000, 8], 72)
    assert st == 0 and n > 0
    assert _ws(lib, [3, 2], [10, 8], 8193)[0] == INVALID_VALUE         # alphabet over the build's limit (what compute_ctc_loss refuses)
    st, n = _ws(lib, [3, 2], [10, 8], 8192)
    assert st == 0 and n > 0
    size = ctypes.c_size_t(0)
    ll = (ctypes.c_int * 1)(1)
    assert lib.get_workspace_size(None, ll, 72, 1, Opt(None, 0), ctypes.byref(size)) == INVALID_VALUE
    assert lib.get_workspace_size(ll, None, 72, 1, Opt(None, 0), ctypes.byref(size)) == INVALID_VALUE
    assert lib.get_workspace_size(ll, ll, 72, 1, Opt(None, 0), None) == INVALID_VALUE


def test_workspace_size_grows_with_the_problem(lib):
    st, base = _ws(lib, [5, 3], [40, 30], 72)
    assert st == 0 and base > 0
    assert _ws(lib, [5, 3], [40, 30], 72, blank=7) == (0, base)   # the blank does not change the size
    for ll, il, V in [([5, 3, 4], [40, 30, 20], 72),               # more utterances
                      ([9, 3], [40, 30], 72),                      # longer labels
                      ([5, 3], [80, 30], 72),                      # more frames
                      ([5, 3], [40, 30], 500),                     # larger alphabet
                      ([5, 3], [40, 31], 72)]:                    # one longer utterance
        st, n = _ws(lib, ll, il, V)
        assert st == 0 and n >= base, (ll, il, V, n, base)
    prev = 0
    for B in (1, 2, 8, 64, 256):
        st, n = _ws(lib, [20] * B, [300] * B, 72)
        assert st == 0 and n >= prev
        prev = n


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_ctc.c"
    src.write_text('#include "ctc.h"\n#include <string.h>\n'
                   'size_t probe(void) { struct ctcOptions o; memset(&o, 0, sizeof o); o.blank_label = 3;\n'
                   '  ctcStatus_t s = CTC_STATUS_UNKNOWN_ERROR; (void)s; (void)ctcGetStatusString;\n'
                   '  (void)compute_ctc_loss; (void)get_workspace_size; return sizeof(struct ctcOptions); }\n')
    cc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else (shutil.which("cc") or shutil.which("gcc"))
    if cc is None:
        pytest.skip("no C compiler")
    args = [cc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_options_struct_size_matches_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include "ctc.h"\nsize_t ctc_options_size(void) { return sizeof(struct ctcOptions); }\n'
                   'size_t ctc_options_blank_offset(void) { return offsetof(struct ctcOptions, blank_label); }\n')
    so = tmp_path / "libsize.so"
    subprocess.run([gcc, "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    m = ctypes.CDLL(str(so))
    m.ctc_options_size.restype = m.ctc_options_blank_offset.restype = ctypes.c_size_t
    assert m.ctc_options_size() == ctypes.sizeof(Opt)
    assert m.ctc_options_blank_offset() == Opt.blank_label.offset


def test_compute_ctc_loss_refuses_alphabet_over_the_limit_on_the_host(lib):
    """alphabet_size > 8192 is refused before the first HIP call: the arguments here are HOST buffers, which a call that went on would
    hand to hipMemcpyAsync / the kernels (no GPU needed -- the status and the message show which check answered)."""
    import ctc_crf
    ip = ctypes.POINTER(ctypes.c_int)
    lib.compute_ctc_loss.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ip, ip, ip, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                     ctypes.c_void_p, Opt]
    lib.compute_ctc_loss.restype = ctypes.c_int
    V, B, T = 8193, 2, 4
    act = (ctypes.c_float * (T * B * V))()
    grads = (ctypes.c_float * (T * B * V))()
    labels, ll, il = (ctypes.c_int * 2)(1, 2), (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 2)(T, T)
    costs = (ctypes.c_float * B)(-7.0, -7.0)
    ws = (ctypes.c_char * 4096)()
    st = lib.compute_ctc_loss(ctypes.addressof(act), ctypes.addressof(grads), labels, ll, il, V, B, costs, ctypes.addressof(ws), Opt(None, 0))
    assert st == INVALID_VALUE
    assert "8192" in ctc_crf._C._lib.crf_last_error().decode()
    assert list(costs) == [-7.0, -7.0]
