"""CPU checks of the optimiser calls (gnn.cpp_amd/csrc/gnnx_optim.hip): the new C-ABI entries are declared, exported and bound; every
refusal of include/gnnx.h returns its status before a device is touched; gnnx_adam_bias_corrections (host only) against its
definition; and the Python surface: _Model.step and every train_step keep their parameter lists, set_optimizer reaches every view."""
import ctypes as C
import importlib
import inspect
import os

import numpy as np
import pytest

from tests.helpers import ROOT

INVALID, WORKSPACE, UNSUPPORTED = -1, -4, -7
NEW = {"gnnx_optim_table_bytes": 2, "gnnx_optim_table_build": 9, "gnnx_adam_bias_corrections": 5, "gnnx_adam_step_f32": 15,
       "gnnx_momentum_step_f32": 12, "gnnx_grad_sqnorm_workspace": 1, "gnnx_grad_sqnorm_f32": 8}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("gnncpp_amd.capi")


def test_symbols_are_declared_exported_and_bound(capi):
    L = capi.lib()
    names = capi.declared_symbols()
    for name, n_args in NEW.items():
        assert name in names and hasattr(L, name) and len(capi._SIGS[name]) == n_args, name
    assert "gnnx_optim.hip" in open(os.path.join(ROOT, "gnn.cpp_amd", "csrc", "Makefile")).read()
    header = open(capi.HEADER_PATH).read()
    for line in ("m' = b1 * m + (1.0f - b1) * g2", "v' = b2 * v + ((1.0f - b2) * g2) * g2", "u  = (m' / c1) / (sqrtf(v' / c2) + eps)",
                 "p1 = p - (lr * wd) * p", "buf' = g2 if first else momentum * buf + (1.0f - dampening) * g2",
                 "min(1, max_norm / (sqrtf(sq) + 1e-6f))"):
        assert line in header, line


def test_table_queries_and_refusals_without_device(capi):
    L = capi.lib()
    b = C.c_size_t(0)
    assert L.gnnx_optim_table_bytes(0, C.byref(b)) == 0 and b.value == 16          # first[0 .. 0] alone, rounded up to 16
    assert L.gnnx_optim_table_bytes(9, C.byref(b)) == 0 and b.value == 336         # 9 * 32 + 10 * 4 = 328
    assert L.gnnx_optim_table_bytes(-1, C.byref(b)) == INVALID and L.gnnx_optim_table_bytes(3, None) == INVALID
    assert L.gnnx_grad_sqnorm_workspace(C.byref(b)) == 0 and b.value == 1024 and L.gnnx_grad_sqnorm_workspace(None) == INVALID

    chunks, elems = C.c_int64(-5), C.c_int64(-5)
    fake = 4096       # never dereferenced

    def build(sizes=(5, 0, 7), params=None, grads=None, table=C.c_void_p(fake), nbytes=1 << 20, n=None, out=(chunks, elems), arrays=True):
        k = len(sizes)
        ps = (C.c_void_p * k)(*([fake] * k if params is None else params))
        gs = (C.c_void_p * k)(*([fake] * k if grads is None else grads))
        sz = (C.c_int64 * k)(*sizes)
        return L.gnnx_optim_table_build(k if n is None else n, ps if arrays else None, gs if arrays else None, sz if arrays else None, table, nbytes,
                                        C.byref(out[0]) if out[0] is not None else None, C.byref(out[1]) if out[1] is not None else None, None)

    assert build(n=-1) == INVALID and build(arrays=False) == INVALID
    assert build(sizes=(5, -1, 7)) == INVALID
    assert build(params=[fake, None, None]) == INVALID and build(grads=[None, fake, fake]) == INVALID
    assert b"null" in L.gnnx_last_error()
    assert build(params=[fake, None, fake + 2]) == INVALID            # not 4-byte aligned
    assert build(out=(None, elems)) == INVALID and build(out=(chunks, None)) == INVALID
    assert build(table=None) == INVALID and build(table=C.c_void_p(fake + 4)) == INVALID
    assert build(nbytes=3 * 32 + 4 * 4 - 1) == WORKSPACE
    # 2^31 chunks of 1024 elements and more: refused; one chunk fewer passes the check (and is refused for its table pointer here)
    assert build(sizes=(1 << 41,)) == UNSUPPORTED and build(sizes=(1 << 40, 1 << 40, 1)) == UNSUPPORTED
    assert build(sizes=((1 << 41) - 1024,), table=None) == INVALID
    assert chunks.value == -5 and elems.value == -5                     # a refused call writes nothing


def test_step_refusals_without_device(capi):
    L = capi.lib()
    p = C.c_void_p(4096)

    def adam(table=p, n=3, chunks=3, m=p, v=p, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, c1=0.1, c2=0.001, wd=0.0, dec=0, scale=None):
        return L.gnnx_adam_step_f32(table, n, chunks, m, v, lr, b1, b2, eps, c1, c2, wd, dec, scale, None)

    for name in ("table", "m", "v"):
        assert adam(**{name: None}) == INVALID, name
    assert adam(n=-1) == INVALID and adam(chunks=-1) == INVALID and adam(chunks=1 << 31) == UNSUPPORTED
    assert adam(table=C.c_void_p(4100)) == INVALID
    for name in ("b1", "b2"):
        for bad in (1.0, -0.1, 1.5, float("nan")):
            assert adam(**{name: bad}) == INVALID, (name, bad)
    for name in ("eps", "c1", "c2"):
        for bad in (0.0, -1e-8, float("nan")):
            assert adam(**{name: bad}) == INVALID, (name, bad)
    assert adam(chunks=0, m=None, v=None) == 0 and adam(n=0, chunks=0) == 0      # nothing to do needs no device

    def mom(table=p, n=3, chunks=3, buf=p):
        return L.gnnx_momentum_step_f32(table, n, chunks, buf, 0.01, 0.9, 0.0, 0, 1, 0.0, None, None)

    assert mom(table=None) == INVALID and mom(buf=None) == INVALID and mom(n=-1) == INVALID and mom(chunks=-1) == INVALID
    assert mom(chunks=1 << 31) == UNSUPPORTED and mom(chunks=0, buf=None) == 0

    def norm(table=p, n=3, mx=1.0, sq=p, sc=p, ws=p, wsb=1024):
        return L.gnnx_grad_sqnorm_f32(table, n, mx, sq, sc, ws, wsb, None)

    assert norm(table=None) == INVALID and norm(n=-1) == INVALID and norm(sq=None, sc=None) == INVALID
    assert norm(mx=-1.0) == INVALID and norm(mx=float("nan")) == INVALID
    assert norm(ws=None) == WORKSPACE and norm(wsb=1023) == WORKSPACE


def test_bias_corrections_are_the_definition(capi):
    L = capi.lib()
    for b in (0.9, 0.999, 0.0):
        for t in (1, 2, 10, 1000):
            c1, c2 = C.c_float(-1), C.c_float(-1)
            assert L.gnnx_adam_bias_corrections(b, 0.5, t, C.byref(c1), C.byref(c2)) == 0
            assert np.float32(c1.value) == np.float32(1.0 - float(np.float32(b)) ** t), (b, t)
            assert np.float32(c2.value) == np.float32(1.0 - 0.5 ** t)
    c = C.c_float(-1)
    assert L.gnnx_adam_bias_corrections(0.9, 0.999, 0, C.byref(c), C.byref(c)) == INVALID
    assert L.gnnx_adam_bias_corrections(1.0, 0.999, 1, C.byref(c), C.byref(c)) == INVALID
    assert L.gnnx_adam_bias_corrections(0.9, -0.5, 1, C.byref(c), C.byref(c)) == INVALID
    assert L.gnnx_adam_bias_corrections(0.9, 0.999, 1, None, C.byref(c)) == INVALID and c.value == -1


def test_python_surface():
    ops = importlib.import_module("gnncpp_amd.ops")

    def params(f):
        return list(inspect.signature(f).parameters)

    def default(f, name):
        return inspect.signature(f).parameters[name].default

    # today's parameter lists
    assert params(ops._Model.step) == ["self", "lr", "weight_decay"] and default(ops._Model.step, "weight_decay") == 0.0
    assert params(ops._Stack.train_step) == ["self", "X", "target", "rows", "lr", "weight_decay"]
    assert params(ops.GcnStack.link_train_step) == ["self", "X", "edges", "lr", "weight_decay"]
    assert params(ops.GraphClassifier.train_step) == ["self", "X", "target", "lr", "weight_decay"]
    for cls in (ops.GcnStack, ops.GatStack, ops.SageStack, ops.GraphClassifier):
        assert cls.step is ops._Model.step and cls.set_optimizer is ops._Model.set_optimizer
    for f in (ops._Stack.train_step, ops.GcnStack.link_train_step, ops.GraphClassifier.train_step):
        assert "step of the model's optimiser (plain SGD by default)" in " ".join(f.__doc__.split())
    assert params(ops.Adam.__init__) == ["self", "betas", "eps", "decoupled", "max_grad_norm"]
    assert (default(ops.Adam.__init__, "betas"), default(ops.Adam.__init__, "eps"), default(ops.Adam.__init__, "decoupled"),
            default(ops.Adam.__init__, "max_grad_norm")) == ((0.9, 0.999), 1e-8, False, None)
    assert params(ops.Momentum.__init__) == ["self", "momentum", "dampening", "nesterov", "max_grad_norm"]
    assert (default(ops.Momentum.__init__, "momentum"), default(ops.Momentum.__init__, "dampening"), default(ops.Momentum.__init__, "nesterov")) == (0.9, 0.0, False)
    # the betas are rounded to float32 once; an unbound optimiser has an empty state and t = 0
    a = ops.Adam()
    assert a.b1 == float(np.float32(0.9)) and a.b2 == float(np.float32(0.999)) and a.state() == dict(m=[], v=[], t=0)
    assert ops.Momentum().state() == dict(buf=[], t=0)
    for bad in (dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            ops.Adam(**bad)


def test_set_optimizer_reaches_views_made_before_and_after():
    """The optimiser's slot is shared by _view: one optimiser, whichever model it was set through."""
    ops = importlib.import_module("gnncpp_amd.ops")

    class Toy(ops._Model):
        def __init__(self):
            self._buf, self._saved, self._opt = {}, None, [None]

    net = Toy()
    before = net._view()
    opt = ops.Adam()
    assert net.set_optimizer(opt) is net
    after = net._view(share_buf=True)
    assert before.optimizer is opt and after.optimizer is opt and net.optimizer is opt
    assert after.set_optimizer(None) is after and net.optimizer is None and before.optimizer is None
    with pytest.raises(TypeError):
        net.set_optimizer("adam")
