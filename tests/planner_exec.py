"""TEST / BENCH INFRASTRUCTURE (not product code; the product is librmhip.so behind include/rmhip.h).

Host-side executors: mirror of crates/runmat-accelerate/src/fusion_exec.rs, i.e. what sits between the VM and the
provider calls.  All seven executors of that file are restated here, each with the provider calls in the reference's order:

    execute_elementwise            :196-462   (shared body `execute_elementwise_outputs`)
    execute_reduction              :464-628
    execute_centered_gram          :630-673
    execute_power_step_normalize   :675-729
    execute_explained_variance     :731-868
    execute_image_normalize        :870-952
    execute_matmul_epilogue        :954-1206

The first two resolve the output shape (plan shape or runtime broadcast, trailing-aligned, :216-277), upload host
operands and scalars (scalars become 1-element tensors shaped [1,1,...], :279-353), generate the request text, call
the provider and free the temporaries they uploaded themselves (:415-419).  The five special-pattern executors take
their operands through `ensure_gpu_tensor` (:111-127): a resident handle is borrowed, a host tensor is uploaded and
freed afterwards.  Values may be `GpuTensorHandle`s (resident operands), numpy arrays (host tensors) or Python
floats/ints (Value::Num / Value::Int).

`CallRecorder` wraps any provider (the device one or the CPU double of oracle_provider.py) and keeps the order of the
calls and the handles they created and freed, so that a test can account for every buffer of a sequence.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from planner_requests import FusionGroupPlan
from runmat_amd.provider import GpuTensorHandle, ProviderError, ReductionFlavor

ERR_INVALID = 1
ERR_UNSUPPORTED = 2
ERR_SHAPE = 3


def runtime_broadcast_shape(values: Sequence) -> Optional[Tuple[int, ...]]:
    """fusion_exec.rs:216-245: scalars contribute an empty shape; shapes align on trailing dims."""
    shapes: List[Tuple[int, ...]] = []
    for v in values:
        if isinstance(v, GpuTensorHandle):
            shapes.append(tuple(v.shape))
        elif isinstance(v, np.ndarray):
            shapes.append(tuple(v.shape))
        elif isinstance(v, (int, float)):
            shapes.append(())
        else:
            return None
    rank = max((len(s) for s in shapes), default=0)
    out = [1] * rank
    for shape in shapes:
        offset = rank - len(shape)
        for i, dim in enumerate(shape):
            j = offset + i
            a, b = out[j], dim
            if a == 1:
                out[j] = max(b, 1)
            elif b == 1 or a == b:
                pass
            else:
                return None
    return tuple(out)


def normalize_scalar_shape(shape: Sequence[int]) -> Tuple[int, ...]:
    """Scalars are at least 2-D ([1,1]) like MATLAB values."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 0:
        return (1, 1)
    if len(shape) == 1:
        return (shape[0], 1) if shape[0] != 1 else (1, 1)
    return shape


def _scalar_ty(prov) -> str:
    """`scalar_ty` follows the provider's precision (fusion_exec.rs:262-266)."""
    return "f32" if prov.precision() == "F32" else "f64"


def _prepare(prov, values, scalar_shape):
    prepared, owned = [], []
    for v in values:
        if isinstance(v, GpuTensorHandle):
            prepared.append(v)
        elif isinstance(v, np.ndarray):
            h = prov.upload(np.asarray(v, dtype=np.float64).reshape(-1, order="F"), v.shape if v.ndim else (1, 1))
            prepared.append(h)
            owned.append(h)
        elif isinstance(v, (int, float)):
            h = prov.upload(np.array([float(v)]), scalar_shape)
            prepared.append(h)
            owned.append(h)
        else:
            raise ProviderError(ERR_UNSUPPORTED, "fusion: unsupported value type")
    return prepared, owned


def execute_elementwise(prov, plan: FusionGroupPlan, output_ids: Sequence[int], values: Sequence,
                        plan_shape: Optional[Sequence[Optional[int]]] = None) -> List[GpuTensorHandle]:
    """Returns one resident handle per requested output id (first = the plan's final output)."""
    if len(values) != len(plan.inputs):
        raise ProviderError(1, f"fusion input mismatch: expected {len(plan.inputs)}, got {len(values)}")
    rt = runtime_broadcast_shape(values)
    if plan_shape and all(d is not None for d in plan_shape):
        out_shape = tuple(int(d) for d in plan_shape)
    elif plan_shape and rt is not None and len(rt) == len(plan_shape):
        out_shape = tuple(int(p) if p is not None else r for p, r in zip(plan_shape, rt))
    else:
        if rt is None:
            raise ProviderError(ERR_UNSUPPORTED, "fusion: unknown output shape")
        out_shape = rt
    length = int(np.prod(out_shape, dtype=np.int64)) if len(out_shape) else 1
    if length == 0:
        raise ProviderError(ERR_UNSUPPORTED, "fusion: zero-length execution not supported")
    out_shape = normalize_scalar_shape(out_shape)
    scalar_shape = normalize_scalar_shape([1] * len(out_shape))
    prepared, owned = _prepare(prov, values, scalar_shape)
    try:
        shader = plan.generate_wgsl_for_outputs(list(output_ids), _scalar_ty(prov))
        if len(output_ids) == 1:
            outs = [prov.fused_elementwise(shader, prepared, out_shape, length)]
        else:
            outs = prov.fused_elementwise_multi(shader, prepared, out_shape, length, len(output_ids))
    finally:
        for h in owned:
            prov.free(h)
    return outs


def execute_reduction(prov, plan: FusionGroupPlan, data_vid: int, values: Sequence, reduce_len: int, num_slices: int,
                      axis: int = 0, omitnan: bool = False, flavor: Optional[ReductionFlavor] = None,
                      workgroup_size: int = 256) -> GpuTensorHandle:
    """fusion_exec.rs:464-628: output shape is [num_slices]; geometry comes from the VM
    (crates/runmat-vm/src/accel/fusion.rs:540-915)."""
    if reduce_len * num_slices == 0:
        raise ProviderError(ERR_UNSUPPORTED, "fusion: zero-length execution not supported")
    flavor = flavor or ReductionFlavor.Sum()
    prepared, owned = _prepare(prov, values, (1, 1))
    try:
        shader = plan.generate_reduction_wgsl(data_vid, _scalar_ty(prov), axis=axis, omitnan=omitnan, is_mean=flavor.kind == "mean")
        wg = workgroup_size or prov.default_reduction_workgroup_size()
        return prov.fused_reduction(shader, prepared, (num_slices,), reduce_len, num_slices, wg, flavor)
    finally:
        for h in owned:
            prov.free(h)


# ---- special fusion patterns ------------------------------------------------------------------------------------------
class CallRecorder:
    """Forwards every call to `prov` and records it: `calls` is the order of the method names, `log` the same with the
    arguments, `created` the handles that calls returned (a `reshape` returns its operand's id again and creates nothing),
    `freed` the ids handed to `free`."""

    def __init__(self, prov):
        self._prov = prov
        self.calls: List[str] = []
        self.log: List[tuple] = []
        self.created: List[GpuTensorHandle] = []
        self.freed: List[int] = []

    def __getattr__(self, name):
        target = getattr(self._prov, name)
        if not callable(target):
            return target

        def call(*args, **kwargs):
            self.calls.append(name)
            self.log.append((name, args, kwargs))
            out = target(*args, **kwargs)
            if name == "free":
                self.freed.append(args[0].buffer_id)
            elif name != "reshape" and isinstance(out, GpuTensorHandle):
                self.created.append(out)
            return out

        return call


def ensure_gpu_tensor(prov, value) -> Tuple[GpuTensorHandle, Optional[GpuTensorHandle]]:
    """fusion_exec.rs:111-127: (handle, the same handle again when this call uploaded it and the caller must free it)."""
    if isinstance(value, GpuTensorHandle):
        return value, None
    if isinstance(value, np.ndarray):
        a = np.asarray(value, dtype=np.float64)
        h = prov.upload(a.reshape(-1, order="F"), a.shape if a.ndim else (1, 1))
        return h, h
    raise ProviderError(ERR_INVALID, "fusion: expected tensor input")


def _free_all(prov, handles) -> None:
    for h in handles:
        if h is not None:
            try:
                prov.free(h)  # `let _ = provider.free(..)`: a failing free is ignored
            except ProviderError:
                pass


def execute_centered_gram(prov, matrix, normalization: str = "unbiased") -> GpuTensorHandle:
    """fusion_exec.rs:630-673: `covariance(matrix, None, None, {normalization, rows: All, no weights})`, then the owned
    upload is freed.  `normalization` is "unbiased" (N - 1) or "biased" (N)."""
    if normalization not in ("unbiased", "biased"):
        raise ProviderError(ERR_INVALID, "centered gram: missing pattern metadata")
    handle, owned = ensure_gpu_tensor(prov, matrix)
    try:
        return prov.covariance(handle, None, None, biased=normalization == "biased", rows="all")
    finally:
        _free_all(prov, [owned])


def execute_power_step_normalize(prov, lhs, rhs, epsilon: float) -> GpuTensorHandle:
    """fusion_exec.rs:675-729: lhs, then rhs through `ensure_gpu_tensor`, `matmul_power_step(lhs, rhs, {epsilon})`, the
    owned uploads freed lhs first."""
    lhs_handle, lhs_owned = ensure_gpu_tensor(prov, lhs)
    rhs_owned = None
    try:
        rhs_handle, rhs_owned = ensure_gpu_tensor(prov, rhs)
        return prov.matmul_power_step(lhs_handle, rhs_handle, float(epsilon))
    finally:
        _free_all(prov, [lhs_owned, rhs_owned])


def execute_explained_variance(prov, q, g) -> GpuTensorHandle:
    """fusion_exec.rs:731-868.  `diag((Q' * G) * Q)` as the interpreter computes it: its transpose keeps the data layout,
    so Q is RESHAPED to the swapped shape under its own id (:813-818), multiplied, reshaped back (:830) and multiplied
    again; the diagonal of the product comes back as [len, 1] (:838-843)."""
    q_handle, q_owned = ensure_gpu_tensor(prov, q)
    g_owned = None
    temps: List[GpuTensorHandle] = []
    try:
        g_handle, g_owned = ensure_gpu_tensor(prov, g)
        q_shape = tuple(q_handle.shape)  # :778-794
        if len(q_shape) < 2:
            raise ProviderError(ERR_SHAPE, "explained variance: Q must be 2-D")
        q_rows, q_cols = q_shape[0], q_shape[1]
        if q_rows == 0 or q_cols == 0:
            raise ProviderError(ERR_SHAPE, "explained variance: zero-sized Q")
        g_shape = tuple(g_handle.shape)
        if len(g_shape) < 2:
            raise ProviderError(ERR_SHAPE, "explained variance: G must be 2-D")
        if g_shape[0] != q_rows or g_shape[1] != q_rows:
            raise ProviderError(ERR_SHAPE, "explained variance: G shape mismatch")

        tmp0 = prov.matmul(q_handle, g_handle)  # :796
        # The reference overwrites this handle at :820 without freeing it.  Freed here - the one deviation from the
        # reference's calls - so that a test can account for every buffer of the sequence.
        temps.append(tmp0)
        if len(tmp0.shape) < 2:
            raise ProviderError(ERR_SHAPE, "explained variance: intermediate must be 2-D")
        if tmp0.shape[0] != q_cols:
            raise ProviderError(ERR_SHAPE, f"explained variance: expected intermediate rows {q_cols}, got {tmp0.shape[0]}")

        swapped = (q_shape[1], q_shape[0]) + q_shape[2:]
        q_transposed_view = prov.reshape(q_handle, swapped)  # :816-818, same id
        try:
            tmp = prov.matmul(q_transposed_view, g_handle)  # :820
            temps.append(tmp)
        finally:
            q_handle = prov.reshape(q_handle, q_shape)  # :830 (also on an error: the caller's Q keeps its shape)
        product = prov.matmul(tmp, q_handle)  # :832
        temps.append(product)
        diag = prov.diag_extract(product, 0)  # :838
        if len(diag.shape) == 1:  # :839-843
            diag = prov.reshape(diag, (diag.shape[0], 1))
        return diag
    finally:
        # :857-864 free tmp, product, the owned Q, the owned G in this order; tmp0 (see above) goes last
        _free_all(prov, temps[1:] + [q_owned, g_owned] + temps[:1])


def execute_image_normalize(prov, x, epsilon: float, gain: Optional[float] = None, bias: Optional[float] = None,
                            gamma: Optional[float] = None, clamp_zero: bool = True) -> GpuTensorHandle:
    """fusion_exec.rs:870-952: batch, height and width are the handle's rank-3 shape (:905-914), the scalars are already
    resolved numbers (`resolve_image_scalar_value`, :170-194)."""
    handle, owned = ensure_gpu_tensor(prov, x)
    try:
        shape = tuple(handle.shape)
        if len(shape) != 3:
            raise ProviderError(ERR_SHAPE, f"image normalize: expected 3-D input tensor, got shape {list(shape)}")
        batch, height, width = shape
        return prov.image_normalize(handle, batch, height, width, float(epsilon), gain=gain, bias=bias, gamma=gamma,
                                    clamp_zero=bool(clamp_zero))
    finally:
        _free_all(prov, [owned])


def derive_matmul_epilogue(plan: FusionGroupPlan, handles: Dict[int, GpuTensorHandle], const_values: Dict[int, float]):
    """fusion_exec.rs:992-1159: find the `mtimes` op, then walk ALL operations in order and fold those that consume the
    running value into a descriptor.  Returns (a_vid, b_vid, descriptor keywords of `matmul_epilogue`, diag value id or
    None, the last running value id).  The rules are the reference's accumulation, not algebra: `((A*B)+1)*2` keeps
    alpha = 2 and beta = 1."""
    a_vid = b_vid = cur = None
    for op in plan.operations:
        if op.kind == "builtin" and op.name.lower() == "mtimes":
            a_vid = op.inputs[0] if len(op.inputs) > 0 else None
            b_vid = op.inputs[1] if len(op.inputs) > 1 else None
            cur = op.output
            break
    if a_vid is None or b_vid is None:
        raise ProviderError(ERR_INVALID, "mtimes not found")
    alpha, beta = 1.0, 0.0
    row_scale = col_scale = None
    clamp_min = clamp_max = pow_exponent = None
    row_div = col_div = False
    diag_vid = None

    def scale_operand(other: int, divide: bool):
        nonlocal row_scale, col_scale, row_div, col_div
        if row_scale is not None and col_scale is not None:
            return
        h = handles.get(other)
        if h is None:
            return
        r = h.shape[0] if len(h.shape) > 0 else 1
        c = h.shape[1] if len(h.shape) > 1 else 1
        if c == 1 and row_scale is None:
            row_scale, row_div = h, divide
        elif r == 1 and col_scale is None:
            col_scale, col_div = h, divide

    for op in plan.operations:
        if cur not in op.inputs:
            continue
        if op.kind == "primitive":
            other = op.inputs[1] if op.inputs[0] == cur else op.inputs[0]
            const = const_values.get(other)
            if op.name in ("Mul", "ElemMul"):
                if const is not None:
                    alpha *= const
                else:
                    scale_operand(other, False)
            elif op.name == "ElemDiv":
                if const is not None:
                    if const != 0.0:
                        alpha *= 1.0 / const
                else:
                    scale_operand(other, True)
            elif op.name == "Add":
                if const is not None:
                    beta += const
            elif op.name == "Sub":
                if const is not None:
                    beta -= const
            elif op.name in ("Pow", "ElemPow"):
                if pow_exponent is None and op.inputs[0] == cur:
                    pow_exponent = const
        else:
            lower = op.name.lower()
            other = next((v for v in op.inputs if v != cur), None)
            const = const_values.get(other) if other is not None else None
            if lower in ("max", "min"):
                if const is not None:
                    if lower == "max":
                        clamp_min = const if clamp_min is None else max(clamp_min, const)
                    else:
                        clamp_max = const if clamp_max is None else min(clamp_max, const)
            elif lower == "pow" and pow_exponent is None:
                if const is not None:
                    pow_exponent = const
            elif lower == "diag":
                diag_vid = op.output
        cur = op.output
    desc = dict(alpha=alpha, beta=beta, row_scale=row_scale, col_scale=col_scale,
                row_op="divide" if row_div else "multiply", col_op="divide" if col_div else "multiply",
                clamp_min=clamp_min, clamp_max=clamp_max, pow_exponent=pow_exponent)
    return a_vid, b_vid, desc, diag_vid, cur


def execute_matmul_epilogue(prov, plan: FusionGroupPlan, values: Sequence, const_values: Dict[int, float],
                            output: Optional[int] = None) -> GpuTensorHandle:
    """fusion_exec.rs:954-1206.  `values` are the runtime values of `plan.inputs` (resident handles or host tensors,
    :961-983), `const_values` the plan's constants by value id, `output` the plan's output value id (None: the last
    running value, :1188).  A `diag` op allocates `zeros([min(m, n), 1])` as the descriptor's `diag_output` (:1164-1177);
    when the plan's output is that diag value the matrix result is freed and the diagonal returned (:1188-1205)."""
    handles: Dict[int, GpuTensorHandle] = {}
    owned: List[GpuTensorHandle] = []
    diag_handle = None
    done = False
    try:
        for idx, vid in enumerate(plan.inputs):
            if idx >= len(values):
                raise ProviderError(ERR_INVALID, "fusion: missing input value")
            v = values[idx]
            if isinstance(v, GpuTensorHandle):
                h = v
            elif isinstance(v, np.ndarray):
                h, _ = ensure_gpu_tensor(prov, v)
                owned.append(h)
            else:
                raise ProviderError(ERR_INVALID, "matmul_epilogue: unsupported input value kind")
            handles.setdefault(vid, h)  # `find_handle` takes the first match
        a_vid, b_vid, desc, diag_vid, cur = derive_matmul_epilogue(plan, handles, const_values)
        if a_vid not in handles:
            raise ProviderError(ERR_INVALID, "missing A")
        if b_vid not in handles:
            raise ProviderError(ERR_INVALID, "missing B")
        a, b = handles[a_vid], handles[b_vid]
        if diag_vid is not None:
            diag_len = min(a.shape[0] if len(a.shape) > 0 else 0, b.shape[1] if len(b.shape) > 1 else 0)
            diag_handle = prov.zeros((diag_len, 1))
        out = prov.matmul_epilogue(a, b, diag_output=diag_handle, **desc)
        done = True
    finally:
        _free_all(prov, owned)  # :1180-1182
        if not done:
            _free_all(prov, [diag_handle])  # the reference returns with `?` here; nobody else could free it
    final_vid = output if output is not None else cur
    if diag_handle is not None and diag_vid == final_vid:
        _free_all(prov, [out])  # :1198-1199
        return diag_handle
    return out
