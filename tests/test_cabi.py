"""The C-ABI library loads and exports every symbol include/tsamd.h declares (no compute here),
and the host layer refuses CPU tensors instead of falling back.  CPU only."""
import ctypes
import os
import re

import pytest
import torch

from pytorch_sparse_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'tsamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(tsamd_[a-z0-9_]+)\s*\(', src)))


def test_header_symbols_are_exported():
    """Every prototype is read: this file's regex and the binding's parser, two readers of one header, find the same
    names, and the library exports each of them."""
    syms = declared_symbols()
    assert len(syms) >= 150
    assert sorted(nat.SIGNATURES) == syms == nat.SYMBOLS, 'the binding read other prototypes than the header declares'
    lib = ctypes.CDLL(nat.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), 'libtsamd.so does not export %s' % s


def prototypes():
    """{name: (return type, parameter count)} by a reader of its own: the text up to the name, the commas."""
    src = open(os.path.join(ROOT, 'include', 'tsamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    found = re.findall(r'(\w[\w \t]*?[ *])(tsamd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)
    return {name: (' '.join(ret.split()), 0 if params.strip() == 'void' else params.count(',') + 1)
            for ret, name, params in found}


def test_every_function_carries_its_declaration():
    L, protos = nat.lib(), prototypes()
    assert sorted(protos) == declared_symbols()
    restypes = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64, 'const char *': ctypes.c_char_p}
    for name, (ret, nparams) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restypes[ret], name
        assert len(fn.argtypes) == nparams, name
    assert sum(ret == 'size_t' for ret, _ in protos.values()) >= 38
    assert sorted(n for n, (ret, _) in protos.items() if ret == 'int64_t') == ['tsamd_hip_version', 'tsamd_num_diag']
    assert [n for n, (ret, _) in protos.items() if ret == 'const char *'] == ['tsamd_status_string']
    assert L.tsamd_hip_version.argtypes == [] and L.tsamd_status_string.argtypes == [ctypes.c_int]
    # three signatures as literals: between them every scalar kind, `double` + `uint64_t`, and a `float *`
    i, q, vp, sz, dbl, u64 = (ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double,
                              ctypes.c_uint64)
    spmm = [i, i, vp, vp, vp, vp, vp, vp, q, q, q, q, q, vp, sz, vp]
    assert L.tsamd_spmm.argtypes == spmm and L.tsamd_spmm.restype is i
    assert L.tsamd_spmm_profiled.argtypes == spmm + [vp]
    assert L.tsamd_attention_heads_dropout.argtypes == [i, vp, vp, vp, q, vp, vp, vp, dbl, dbl, u64, vp, vp, q, q, q, q, q,
                                                        vp, sz, vp]


def test_parser_is_loud_about_what_it_cannot_map():
    ok = 'size_t tsamd_a(int x, const float *y, int64_t z[4]); /* tsamd_not_a_call(...) */\nvoid tsamd_b(void);'
    assert nat.parse_header(ok) == {'tsamd_a': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
                                    'tsamd_b': (None, [])}
    assert nat.parse_header('float tsamd_c(uint32_t n, double x, uint64_t s, float f);')['tsamd_c'] == (
        ctypes.c_float, [ctypes.c_uint32, ctypes.c_double, ctypes.c_uint64, ctypes.c_float])
    for bad in ('int tsamd_c(unsigned n);', 'int tsamd_c(long n);', 'short tsamd_c(int n);', 'int tsamd_c(hipStream_t s);',
                'void *tsamd_c(int n);', 'int tsamd_c(unsigned int n);'):
        with pytest.raises(TypeError, match='tsamd_c'):
            nat.parse_header(bad)
    with pytest.raises(TypeError, match='plain form'):  # a prototype the pattern does not read is not skipped
        nat.parse_header('int tsamd_c(int (*callback)(int), int n);')


def test_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(nat, 'HEADER_PATH', '/nonexistent/tsamd.h')
    with pytest.raises(ImportError, match='no CPU fallback'):
        nat.load_signatures()


def test_wrong_kinds_are_refused():
    """An int64 object for an `int` or `size_t` parameter and a float for an integer are errors, not truncations."""
    L = nat.lib()
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        L.tsamd_status_string(ctypes.c_int64(0))
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        L.tsamd_spmm_workspace_bytes(ctypes.c_int64(0), 0, 1, 10, 10, 16, 100)
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        L.tsamd_spmm_workspace_bytes(0, 0, 1, 10, 10, 16.0, 100)
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        L.tsamd_sort_coo_workspace_bytes(ctypes.c_int(5))
    with pytest.raises((ctypes.ArgumentError, TypeError)):  # and a missing argument
        L.tsamd_spmm_workspace_bytes(0, 0, 1, 10, 10, 16)


STRAY = re.compile(r'\.(argtypes|restype)\s*=[^=]')


def test_no_stray_declarations():
    """No file under tests/ or scripts/ declares a tsamd signature of its own: the header is the one table."""
    hits = []
    for sub in ('tests', 'scripts'):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in sorted(files):
                if not f.endswith('.py'):
                    continue
                rel = os.path.relpath(os.path.join(dirpath, f), ROOT).replace(os.sep, '/')
                for no, line in enumerate(open(os.path.join(dirpath, f)), 1):
                    if STRAY.search(line) and 'c_oracle' not in line:  # (the C oracle is another library)
                        hits.append('%s:%d: %s' % (rel, no, line.strip()))
    assert not hits, hits


def test_version_and_status_strings():
    L = nat.lib()
    assert L.tsamd_hip_version() >= 60000000
    assert L.tsamd_status_string(0) == b'ok'
    assert b'workspace' in L.tsamd_status_string(4)
    # workspace query is host-only arithmetic
    i64 = ctypes.c_int64
    assert L.tsamd_spmm_workspace_bytes(0, 0, i64(1), i64(10), i64(10), i64(16), i64(100)) > 0
    assert L.tsamd_spmm_workspace_bytes(99, 0, i64(1), i64(10), i64(10), i64(16), i64(100)) == 0


def test_no_cpu_fallback():
    rowptr, col = torch.tensor([0, 1]), torch.tensor([0])
    with pytest.raises(nat.TsamdError, match='no CPU implementation'):
        nat.spmm(rowptr, col, None, torch.ones(1, 4), 'sum')
    with pytest.raises(nat.TsamdError):
        nat.ind2ptr(torch.tensor([0, 1]), 3)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(nat, '_lib', None)
    monkeypatch.setattr(nat, 'LIB_PATH', '/nonexistent/libtsamd.so')
    with pytest.raises(ImportError, match='no CPU fallback'):
        nat.lib()


def test_argument_validation_returns_status_codes():
    """Bad arguments are rejected by the C-ABI before any HIP call (so this runs without a GPU)."""
    L = nat.lib()
    i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    fake = vp(0x1000)  # never dereferenced: every call below fails validation first
    # negative size / unknown reduce / unknown dtype / N too large
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, i64(1), i64(-1), i64(4), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 1
    assert L.tsamd_spmm(0, 7, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 2
    assert L.tsamd_spmm(42, 0, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 2
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(1 << 33), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 2
    # null pointers; min/max without arg_out; workspace missing / too small / misaligned
    assert L.tsamd_spmm(0, 0, None, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 1
    assert L.tsamd_spmm(0, 3, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        fake, sz(1 << 20), None) == 1
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        None, sz(0), None) == 4
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        fake, sz(16), None) == 4
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, i64(1), i64(4), i64(4), i64(4), i64(4),
                        vp(0x1008), sz(1 << 20), None) == 4
    # nothing to do is OK without touching anything
    assert L.tsamd_spmm(0, 0, None, None, None, None, None, None, i64(1), i64(0), i64(4), i64(4), i64(0),
                        None, sz(0), None) == 0
    # backward entry points
    assert L.tsamd_spmm_value_bw(0, 2, None, fake, fake, fake, fake, fake, i64(1), i64(4), i64(4), i64(4),
                                 i64(4), None) == 2  # only sum / mean have a value gradient
    assert L.tsamd_spmm_value_bw(4, 0, None, fake, fake, fake, fake, fake, i64(1), i64(4), i64(4), i64(4),
                                 i64(4), None) == 2  # integer dtypes have no gradient
    assert L.tsamd_spmm_minmax_bw(5, fake, fake, None, fake, fake, fake, fake, fake, i64(1), i64(4), i64(4), i64(4),
                                  i64(4), None, sz(0), None) == 2
    assert L.tsamd_ind2ptr(None, i64(4), i64(3), fake, None) == 1
    assert L.tsamd_sort_coo(fake, fake, i64(5), i64(1 << 40), i64(1 << 40), None, None, fake, fake,
                            sz(1 << 30), None) == 2  # keys would not fit 63 bits
    assert L.tsamd_sort_coo(fake, fake, i64(5), i64(9), i64(9), None, None, fake, None, sz(0), None) == 4
    assert L.tsamd_segment_reduce(0, 9, fake, None, fake, i64(3), i64(1), fake, None) == 2
    assert L.tsamd_spspmm_numeric(2, fake, fake, None, fake, fake, None, i64(4), i64(4), fake, fake, i64(0),
                                  i64(0), i64(0), fake, fake, None, 0, None, sz(0), None) == 2  # f16: like torch.sparse.mm
    assert L.tsamd_spspmm_symbolic(0, fake, fake, None, fake, fake, None, 0, i64(4), i64(4), fake, fake, i64(0), i64(1),
                                   i64(9000), fake, None, sz(0), None) == 4  # rows beyond the LDS capacity need the workspace
    # workspace sizes grow with the problem and include the relabel copy only when it can pay off
    small = L.tsamd_spmm_workspace_bytes(0, 0, i64(1), i64(1000), i64(1000), i64(128), i64(5000))
    big = L.tsamd_spmm_workspace_bytes(0, 0, i64(1), i64(1 << 21), i64(1 << 21), i64(128), i64(40 << 20))
    halo = L.tsamd_spmm_workspace_bytes(0, 0, i64(1), i64(1 << 21), i64(1 << 24), i64(128), i64(40 << 20))
    assert small < (1 << 22) and big > (1 << 30) and halo < (1 << 28)


def test_plain_ints_are_not_truncated():
    """The host-only checks above with bare Python ints: the declarations carry every width, so the statuses and sizes are
    those of the fully wrapped calls."""
    L = nat.lib()
    i64 = ctypes.c_int64
    fake = 0x1000
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, -1, 4, 4, 4, fake, 1 << 20, None) == 1
    assert L.tsamd_spmm(0, 7, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, fake, 1 << 20, None) == 2
    assert L.tsamd_spmm(42, 0, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, fake, 1 << 20, None) == 2
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, 4, 1 << 33, 4, 4, fake, 1 << 20, None) == 2
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, 4, (1 << 33) + 4, 4, 4, fake, 1 << 20, None) == 2
    assert L.tsamd_spmm(0, 0, None, fake, None, fake, fake, None, 1, 4, 4, 4, 4, fake, 1 << 20, None) == 1
    assert L.tsamd_spmm(0, 3, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, fake, 1 << 20, None) == 1
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, None, 0, None) == 4
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, fake, 16, None) == 4
    assert L.tsamd_spmm(0, 0, fake, fake, None, fake, fake, None, 1, 4, 4, 4, 4, 0x1008, 1 << 20, None) == 4
    assert L.tsamd_spmm(0, 0, None, None, None, None, None, None, 1, 0, 4, 4, 0, None, 0, None) == 0
    assert L.tsamd_spmm_value_bw(0, 2, None, fake, fake, fake, fake, fake, 1, 4, 4, 4, 4, None) == 2
    assert L.tsamd_spmm_value_bw(4, 0, None, fake, fake, fake, fake, fake, 1, 4, 4, 4, 4, None) == 2
    assert L.tsamd_spmm_minmax_bw(5, fake, fake, None, fake, fake, fake, fake, fake, 1, 4, 4, 4, 4, None, 0, None) == 2
    assert L.tsamd_ind2ptr(None, 4, 3, fake, None) == 1
    assert L.tsamd_sort_coo(fake, fake, 5, 1 << 40, 1 << 40, None, None, fake, fake, 1 << 30, None) == 2
    assert L.tsamd_sort_coo(fake, fake, 5, 9, 9, None, None, fake, None, 0, None) == 4
    assert L.tsamd_segment_reduce(0, 9, fake, None, fake, 3, 1, fake, None) == 2
    assert L.tsamd_spspmm_numeric(2, fake, fake, None, fake, fake, None, 4, 4, fake, fake, 0, 0, 0, fake, fake, None, 0, None,
                                  0, None) == 2
    assert L.tsamd_spspmm_symbolic(0, fake, fake, None, fake, fake, None, 0, 4, 4, fake, fake, 0, 1, 9000, fake, None, 0,
                                   None) == 4
    for args in ((0, 0, 1, 1000, 1000, 128, 5000), (0, 0, 1, 1 << 21, 1 << 21, 128, 40 << 20),
                 (0, 0, 1, 1 << 21, 1 << 24, 128, 40 << 20)):
        wrapped = L.tsamd_spmm_workspace_bytes(args[0], args[1], *(i64(a) for a in args[2:]))
        assert L.tsamd_spmm_workspace_bytes(*args) == wrapped > 0
    assert L.tsamd_spmm_workspace_bytes(0, 0, 1, 1 << 21, 1 << 21, 128, 40 << 20) > 1 << 30
    # an answer beyond 2^32 from host arithmetic alone: the sort's workspace at 2^30 entries, the value the fully wrapped
    # call (c_int64 argument, restype c_size_t) gave before the declarations came from the header
    assert L.tsamd_sort_coo_workspace_bytes(1 << 30) == 34718350080 == L.tsamd_sort_coo_workspace_bytes(i64(1 << 30))
    # a query no file declared before (its answer came back as a C int: 256 here) with an argument beyond 32 bits
    assert L.tsamd_coalesce_workspace_bytes(1 << 40) == (1 << 32) + 256


def _build_c_example(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, 'pytorch_sparse_amd', 'lib')
    exe = str(tmp_path / 'spmm_cabi')
    cmd = ['gcc', '-std=c99', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__', os.path.join(root, 'examples', 'spmm_cabi.c'),
           '-I' + os.path.join(root, 'include'), '-I/opt/rocm/include', '-L' + libdir, '-ltsamd', '-L/opt/rocm/lib',
           '-lamdhip64', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-o', exe]
    subprocess.check_call(cmd)
    return exe


def test_plain_c_client_builds(tmp_path):
    """examples/spmm_cabi.c -- C99, gcc, no torch, no C++ -- compiles and links against
    include/tsamd.h + libtsamd.so: the boundary really is a C-ABI."""
    assert os.path.exists(_build_c_example(tmp_path))


@pytest.mark.gpu
def test_plain_c_client_runs(tmp_path):
    import subprocess
    out = subprocess.run([_build_c_example(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'C-ABI example OK' in out.stdout
