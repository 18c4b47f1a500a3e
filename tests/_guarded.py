"""Device buffers for the element-by-element GPU tests: the data is the middle of a larger buffer pre-filled with
a sentinel whose bits must be unchanged after the call, and an output holds NaN before it."""
import numpy as np

SENTINEL = 0x7FF8DEAD0000BEEF        # a NaN with a payload: no kernel produces these bits
GUARD = 8                            # sentinels in front of and behind the data


class Guarded(object):
    """n doubles in the middle of a sentinel-filled buffer; data=None: NaN (an output).  cm: a namespace with
    torch and D (cosmomap2_amd.device)"""

    def __init__(self, cm, n, data=None):
        torch = cm.torch
        self.cm, self.n = cm, int(n)
        self.buf = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.int64,
                              device=cm.D.dev()).view(torch.float64)
        self.v = self.buf[GUARD:GUARD + self.n]
        if data is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(cm.D.to_dev(np.ascontiguousarray(data, dtype=np.float64).reshape(-1)))

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        self.cm.torch.cuda.synchronize()
        return self.v.cpu().numpy().copy()

    def intact(self, what):
        raw = self.buf.view(self.cm.torch.int64)
        assert bool((raw[:GUARD] == SENTINEL).all().item()) and \
            bool((raw[GUARD + self.n:] == SENTINEL).all().item()), \
            "%s: wrote outside its %d elements" % (what, self.n)


INT_GUARD = {"int32": 0x5EADBEEF, "uint8": 0xA5, "int64": 0x5EADBEEF0000BEEF}      # guard sentinels per dtype
INT_FILL = {"int32": -0x5A5A5A5B, "uint8": 0x5A, "int64": -0x5A5A5A5A5A5A5A5B}     # no kernel produces these


class GuardedInt(object):
    """Guarded for n int32 / uint8 / int64 elements (dtype: the name); data=None: INT_FILL[dtype] (an output)"""

    def __init__(self, cm, n, dtype, data=None):
        torch = cm.torch
        self.cm, self.n, self.dtype = cm, int(n), dtype
        self.guard, self.fill = INT_GUARD[dtype], INT_FILL[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.guard, dtype=getattr(torch, dtype), device=cm.D.dev())
        self.v = self.buf[GUARD:GUARD + self.n]
        if data is None:
            self.v.fill_(self.fill)
        else:
            self.v.copy_(cm.D.to_dev(np.ascontiguousarray(data, dtype=np.dtype(dtype)).reshape(-1)))

    @property
    def ptr(self):
        return self.v.data_ptr()

    def get(self):
        self.cm.torch.cuda.synchronize()
        return self.v.cpu().numpy().copy()

    def intact(self, what):
        assert bool((self.buf[:GUARD] == self.guard).all().item()) and \
            bool((self.buf[GUARD + self.n:] == self.guard).all().item()), \
            "%s: wrote outside its %d elements" % (what, self.n)
