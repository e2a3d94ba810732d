"""Test doubles: objects with HipProvider's method names whose arithmetic is the CPU oracle.
`OracleProvider` is used ONLY by the CPU tests of the sharding host logic (world_size-2 gloo), `TableOracleProvider`
ONLY by the CPU twin of the executors' call sequences (test_exec_sequences_host.py); never by the product."""
import numpy as np


class Handle:
    def __init__(self, arr):
        self.arr = np.asarray(arr, dtype=np.float64)
        self.shape = self.arr.shape


class OracleProvider:
    def __init__(self, oracle):
        self.o = oracle
        self.state = oracle.rng_default_seed()

    def upload(self, a, shape=None):
        a = np.asarray(a, dtype=np.float64)
        return Handle(a if shape is None else a.reshape(shape, order="F"))

    def download(self, h):
        return h.arr.reshape(-1, order="F")

    def free(self, h):
        pass

    def fill(self, shape, v):
        return Handle(np.full(shape, float(v)))

    def matmul(self, a, b):
        return Handle(self.o.matmul(a.arr, b.arr))

    def set_rng_state(self, s):
        self.state = int(s)

    def get_rng_state(self):
        return self.state

    def random_normal(self, shape):
        n = int(np.prod(shape))
        z, self.state = self.o.rng_normal(self.state, n)
        return Handle(z.reshape(shape, order="F"))

    def stochastic_evolution(self, h, drift, scale, steps, draws_per_step=0):
        # sharded form of include/rmhip.h: step t draws from state + t * draws_per_step
        x = h.arr.reshape(-1, order="F").copy()
        per = draws_per_step or 2 * ((x.size + 1) // 2)
        base = self.state
        for t in range(steps):
            z, _ = self.o.rng_normal(self.o.rng_advance(base, t * per), x.size)
            x = self.o.binary("mul", x.reshape(-1, 1), self.o.unary("exp", self.o.binary("add", np.array([[float(drift)]]),
                              self.o.binary("mul", np.array([[float(scale)]]), z.reshape(-1, 1))))).reshape(-1)
        self.state = self.o.rng_advance(base, steps * per)
        return Handle(x.reshape(h.arr.shape, order="F"))

    def scalar_mul(self, a, s):
        return Handle(self.o.binary("mul", a.arr, np.array([[float(s)]])))

    def scalar_add(self, a, s):
        return Handle(self.o.binary("add", a.arr, np.array([[float(s)]])))

    def scalar_sub(self, a, s):
        return Handle(self.o.binary("sub", a.arr, np.array([[float(s)]])))

    def scalar_max(self, a, s):
        return Handle(self.o.binary("max", a.arr, np.array([[float(s)]])))

    def unary_exp(self, a):
        return Handle(self.o.unary("exp", a.arr))

    def elem_mul(self, a, b):
        return Handle(self.o.binary("mul", a.arr, b.arr))

    def reduce_sum(self, a):
        return Handle(self.o.reduce_sum(a.arr, "all"))


class TableOracleProvider:
    """The provider as the special-pattern executors of planner_exec.py see it: handles are `GpuTensorHandle`s over a
    buffer table kept here.  One id is one storage (column-major flat data) and the table keeps its shape, so `reshape`
    returns the SAME id with the new shape (lib.rs:2676-2684) and every later call reads the shape of the table, not of
    the handle it was given.  `free` drops the entry: any later use of the id raises the not-found error.  `calls`
    records the method names in order."""

    ERR_INVALID, ERR_UNSUPPORTED, ERR_SHAPE, ERR_NOT_FOUND = 1, 2, 3, 5

    def __init__(self, oracle, device_id: int = 1):
        self.o = oracle
        self._device_id = device_id
        self._table = {}
        self._next = 1
        self.calls = []

    # -- plumbing -----------------------------------------------------------------------------------------------------
    def _err(self, code, msg):
        from runmat_amd.provider import ProviderError
        return ProviderError(code, msg)

    def _new(self, arr):
        from runmat_amd.provider import GpuTensorHandle
        arr = np.asarray(arr, dtype=np.float64)
        bid, self._next = self._next, self._next + 1
        self._table[bid] = [arr.reshape(-1, order="F").copy(), tuple(int(d) for d in arr.shape)]
        return GpuTensorHandle(self._table[bid][1], self._device_id, bid)

    def _entry(self, h, who="buffer"):
        if h.buffer_id not in self._table:
            raise self._err(self.ERR_NOT_FOUND, f"{who} not found: {h.buffer_id}")
        return self._table[h.buffer_id]

    def _arr(self, h):
        flat, shape = self._entry(h)
        return flat.reshape(shape, order="F")

    def live_ids(self):
        return sorted(self._table)

    def precision(self):
        return "F64"

    # -- memory -------------------------------------------------------------------------------------------------------
    def upload(self, data, shape=None):
        self.calls.append("upload")
        a = np.asarray(data, dtype=np.float64)
        if shape is not None:
            if a.size != int(np.prod(shape, dtype=np.int64)):
                raise self._err(self.ERR_SHAPE, "upload: data length does not match shape")
            a = a.reshape(-1).reshape(tuple(shape), order="F")
        elif a.ndim < 2:
            a = a.reshape((a.size, 1) if a.ndim == 1 else (1, 1))
        return self._new(a)

    def download(self, h):
        self.calls.append("download")
        return self._entry(h)[0].copy()

    def download_matrix(self, h):
        self.calls.append("download_matrix")
        return self._arr(h).copy()

    def free(self, h):
        self.calls.append("free")
        if h.buffer_id not in self._table:
            raise self._err(self.ERR_NOT_FOUND, f"free: buffer not found: {h.buffer_id}")
        del self._table[h.buffer_id]

    def zeros(self, shape):
        self.calls.append("zeros")
        return self._new(np.zeros(tuple(shape)))

    def reshape(self, h, shape):
        from runmat_amd.provider import GpuTensorHandle
        self.calls.append("reshape")
        entry = self._entry(h)
        shape = tuple(int(d) for d in shape)
        if int(np.prod(shape, dtype=np.int64)) != entry[0].size:
            raise self._err(self.ERR_SHAPE, f"reshape: element count mismatch ({int(np.prod(shape, dtype=np.int64))} vs {entry[0].size})")
        entry[1] = shape
        return GpuTensorHandle(shape, self._device_id, h.buffer_id)

    # -- the hooks of the special fusion patterns -----------------------------------------------------------------------
    def matmul(self, a, b):
        self.calls.append("matmul")
        A, B = self._arr(a), self._arr(b)
        if A.ndim != 2 or B.ndim != 2:
            raise self._err(self.ERR_UNSUPPORTED, "matmul: only 2D supported")
        if A.shape[1] != B.shape[0]:
            raise self._err(self.ERR_SHAPE, f"matmul: inner dims must agree ({A.shape[0]}x{A.shape[1]} * {B.shape[0]}x{B.shape[1]})")
        return self._new(self.o.matmul(A, B))

    def diag_extract(self, matrix, offset=0):
        self.calls.append("diag_extract")
        M = self._arr(matrix)
        if M.ndim != 2 or M.shape[0] == 1 or M.shape[1] == 1:
            raise self._err(self.ERR_SHAPE, "diag: matrix input required")
        return self._new(np.diagonal(M, offset).reshape(-1, 1))

    def covariance(self, matrix, second=None, weights=None, biased=False, rows="all"):
        self.calls.append("covariance")
        if second is not None or weights is not None or rows != "all":
            raise self._err(self.ERR_UNSUPPORTED, "covariance: second matrix / weights / row filtering use the CPU path")
        return self._new(self.o.covariance(self._arr(matrix), biased))

    def matmul_power_step(self, lhs, rhs, epsilon=0.0):
        self.calls.append("matmul_power_step")
        A, B = self._arr(lhs), self._arr(rhs)
        if A.shape[1] != B.shape[0]:
            raise self._err(self.ERR_SHAPE, "matmul: inner dims must agree")
        return self._new(self.o.matmul_power_step(A, B, epsilon))

    def image_normalize(self, x, batch, height, width, epsilon, gain=None, bias=None, gamma=None, clamp_zero=True):
        self.calls.append("image_normalize")
        X = self._arr(x)
        if X.ndim != 3:
            raise self._err(self.ERR_SHAPE, f"image_normalize: expected 3-D tensor, got rank {X.ndim}")
        if X.shape != (batch, height, width):
            raise self._err(self.ERR_SHAPE, "image_normalize: descriptor dims do not match tensor shape")
        return self._new(self.o.image_normalize(X, epsilon, gain=gain, bias=bias, gamma=gamma, clamp_zero=clamp_zero))

    def matmul_epilogue(self, a, b, alpha=1.0, beta=0.0, row_scale=None, col_scale=None, row_op="multiply",
                        col_op="multiply", clamp_min=None, clamp_max=None, pow_exponent=None, diag_output=None):
        self.calls.append("matmul_epilogue")
        A, B = self._arr(a), self._arr(b)
        if A.shape[1] != B.shape[0]:
            raise self._err(self.ERR_SHAPE, "matmul: inner dims must agree")
        m, n = A.shape[0], B.shape[1]
        rs = self._entry(row_scale)[0] if row_scale is not None else None
        cs = self._entry(col_scale)[0] if col_scale is not None else None
        if rs is not None and rs.size < m:
            raise self._err(self.ERR_SHAPE, f"matmul_epilogue: row scale length {rs.size} < {m} rows")
        if cs is not None and cs.size < n:
            raise self._err(self.ERR_SHAPE, f"matmul_epilogue: col scale length {cs.size} < {n} cols")
        if diag_output is not None and self._entry(diag_output)[0].size < min(m, n):
            raise self._err(self.ERR_SHAPE, "matmul_epilogue: diag_output length insufficient for diag size")
        out, dg = self.o.matmul_epilogue(A, B, alpha=alpha, beta=beta, row_scale=None if rs is None else rs[:m],
                                         col_scale=None if cs is None else cs[:n], row_op=row_op, col_op=col_op,
                                         clamp_min=clamp_min, clamp_max=clamp_max, pow_exponent=pow_exponent,
                                         diag=diag_output is not None)
        if diag_output is not None:
            self._entry(diag_output)[0][: min(m, n)] = dg  # written IN PLACE: the caller's handle now holds the diagonal
        return self._new(out)
