"""
An operator that is dropped goes away at once, by reference count: it does not refer to itself, so the device buffers
it owns are not kept allocated until the cycle collector happens to run (cosmomap2_amd/linop.py).
"""
import gc
import weakref

import numpy as np
import pytest

from cosmomap2_amd import linop as lp
from cosmomap2_amd.interfaces import blkop


class Scale(lp.LinearOperator):
    """Built like the device operators: bound methods of the object itself as matvec and rmatvec."""

    def __init__(self, n, symmetric):
        self.payload = np.full(n, 3.0)
        super(Scale, self).__init__(n, n, self._mult, rmatvec=None if symmetric else self._rmult,
                                    symmetric=symmetric)

    def _mult(self, x):
        return self.payload * x

    def _rmult(self, x):
        return self.payload * x


@pytest.fixture
def no_collector():
    gc.collect()
    gc.disable()
    yield
    gc.enable()


def make(kind):
    if kind == "symmetric":
        return Scale(5, True)
    if kind == "transposable":
        return Scale(5, False)
    if kind == "block":
        return blkop.BlockDiagonalLinearOperator([Scale(2, False), Scale(3, False)])
    return blkop.BlockDiagonalLinearOperator([Scale(2, True), Scale(3, True)])


@pytest.mark.parametrize("kind", ["symmetric", "transposable", "block", "symmetric block"])
def test_a_dropped_operator_is_freed_without_the_cycle_collector(no_collector, kind):
    op = make(kind)
    x = np.arange(5.0)
    np.testing.assert_array_equal(op * x, 3.0 * x)
    np.testing.assert_array_equal(op.T * x, 3.0 * x)
    np.testing.assert_array_equal((op.T * op) * x, 9.0 * x)
    gone = weakref.ref(op)
    del op
    assert gone() is None


def test_the_transpose_keeps_its_operator_and_stays_the_same_object_while_held(no_collector):
    op = Scale(4, False)
    t = op.T
    assert t is op.T and t.T is op and op.T.T is op
    gone = weakref.ref(op)
    del op
    assert gone() is not None                      # the transpose alone still works
    np.testing.assert_array_equal(t * np.ones(4), 3.0 * np.ones(4))
    del t
    assert gone() is None
    s = Scale(4, True)
    assert s.T is s and s._chain == [s]
    p = Scale(4, False).T * Scale(4, False)
    assert len(p._chain) == 2 and p.T.T is p
