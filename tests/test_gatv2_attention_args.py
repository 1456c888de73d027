"""What tsamd_gatv2_* and SparseTensor.gatv2_attention refuse before any device call: through the C entry points with
fake pointers and through Python on CPU tensors.  No GPU."""
import ctypes

import pytest
import torch

from pytorch_sparse_amd import _native as nat

F32, F64, F16, BF16 = 0, 1, 2, 3
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
P = ctypes.c_void_p(4096)  # never dereferenced: every status below is decided on the host
NULL = ctypes.c_void_p(0)


def forward(dtype, H, D, E=10, x_src=P, ws=P, nbytes=1 << 30, M=4):
    return nat.lib().tsamd_gatv2_attention(dtype, P, P, P, x_src, P, 0.2, P, NULL, P, M, 5, H, D, E, ws,
                                           ctypes.c_size_t(nbytes), NULL)


def route(dtype, H, D, E=1000, offs=(0, 0, 0)):
    w = (ctypes.c_int64 * 7)()
    st = nat.lib().tsamd_gatv2_route(dtype, H, D, E, *[ctypes.c_void_p(4096 + o) for o in offs], w)
    return st, [int(v) for v in w]


@pytest.mark.parametrize('dtype,H,D,kw,status', [
    (F16, 2, 8, {}, UNSUPPORTED), (F64, 2, 8, {}, UNSUPPORTED),
    (F32, 2, 257, {}, UNSUPPORTED), (BF16, 2, 513, {}, UNSUPPORTED),   # above 64 * (16 / itemsize)
    (F32, 2, -1, {}, INVALID), (F32, 2, 0, {}, OK),                    # D = 0: out has no element
    (F32, 2, 8, {'M': 1 << 31}, UNSUPPORTED),
    (F32, 2, 8, {'x_src': NULL}, INVALID), (F32, 2, 8, {'ws': NULL}, WORKSPACE), (F32, 2, 8, {'nbytes': 16}, WORKSPACE),
])
def test_forward_status_is_decided_on_the_host(dtype, H, D, kw, status):
    assert forward(dtype, H, D, **kw) == status


def test_backward_and_grad_refusals():
    L = nat.lib()
    bw = lambda dtype, D, lse=P: L.tsamd_gatv2_attention_bw(dtype, NULL, P, P, P, P, P, P, lse, P, 0.2, P, P, 4, 5, 2,  # noqa: E731
                                                            D, 10, NULL)
    assert (bw(F16, 8), bw(F32, 300), bw(F32, 0), bw(F32, 8, NULL)) == (UNSUPPORTED, UNSUPPORTED, INVALID, INVALID)
    grad = lambda dtype, flags, t=P: L.tsamd_gatv2_grad(dtype, flags, P, P, NULL, P, P, P, 0.2, t, NULL, NULL, P, P,  # noqa: E731
                                                         4, 5, 2, 8, 10, P, ctypes.c_size_t(1 << 30), NULL)
    assert (grad(F64, 0), grad(F32, 3), grad(F32, 4), grad(F32, 0, NULL)) == (UNSUPPORTED, UNSUPPORTED, INVALID, INVALID)
    assert grad(F32, 1) == INVALID  # VALUE without p and g


@pytest.mark.parametrize('dtype,item', [(F32, 4), (BF16, 2)])
def test_route_words_and_workspace(dtype, item):
    vec = 16 // item
    for H, D in ((1, 1), (3, 5), (8, 8), (70, 4), (1, 64 * vec)):
        st, w = route(dtype, H, D)
        slots = -(-D // vec)
        lph = 1 << (slots - 1).bit_length()
        hpp = min(1 << (H - 1).bit_length(), 64 // lph)
        assert st == OK and w[:6] == [0 if D % vec == 0 else 1, vec if D % vec == 0 else 1, lph, hpp, -(-H // hpp),
                                      8 * lph * hpp]
        assert w[6] == nat.lib().tsamd_gatv2_workspace_bytes(dtype, H, D, 1000) > 0
    for offs in ((item, 0, 0), (0, item, 0), (0, 0, item)):  # any operand off the boundary: generic, the same lane map
        st, w = route(dtype, 8, 8, offs=offs)
        assert st == OK and w[:2] == [1, 1] and w[2:] == route(dtype, 8, 8)[1][2:]
    assert route(F16, 8, 8)[0] == UNSUPPORTED and route(dtype, 1, 64 * vec + 1)[0] == UNSUPPORTED
    assert nat.lib().tsamd_gatv2_workspace_bytes(F64, 8, 8, 1000) == 0


def test_python_refusals_on_cpu_tensors():
    import pytorch_sparse_amd as ts
    A = ts.SparseTensor(row=torch.tensor([0, 1, 2]), col=torch.tensor([1, 0, 3]), sparse_sizes=(3, 4))
    x = lambda n, *s, dtype=torch.float32: torch.zeros(n, *s, dtype=dtype)  # noqa: E731
    for args, words in [((x(3, 2, 8, dtype=torch.float16), x(4, 2, 8, dtype=torch.float16),
                          x(2, 8, dtype=torch.float16)), 'float32 and bfloat16'),
                        ((x(3, 2, 8, dtype=torch.float64), x(4, 2, 8, dtype=torch.float64),
                          x(2, 8, dtype=torch.float64)), 'float32 and bfloat16'),
                        ((x(3, 2, 0), x(4, 2, 0), x(2, 0)), 'at least one feature'),
                        ((x(3, 1, 257), x(4, 1, 257), x(1, 257)), 'at most 256'),
                        ((x(3, 2, 8), x(4, 2, 4), x(2, 8)), 'value width of its own'),
                        ((x(3, 2, 8), x(4, 2, 8), x(2, 4)), 'att must be')]:
        with pytest.raises(ValueError, match=words):
            A.gatv2_attention(*args)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ts.gatv2_attention(A, x(3, 2, 8), x(4, 2, 8), x(2, 8))
