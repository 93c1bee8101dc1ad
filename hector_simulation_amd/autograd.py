"""``loss.backward()`` through a batched solve: a ``torch.autograd.Function`` over ``BatchedMPC.solve`` whose backward is ONE launch of
the adjoint kernel (include/hector_mpc.h hmpc_solve_adjoint; csrc/hmpc_adjoint.hip).

    forces = differentiable_solve(mpc, fields, traj, weights, alpha_k)     # CUDA float32 [b, h * 6 contacts]
    loss(forces).backward()                                                # traj.grad, weights.grad, alpha_k.grad
    forces = differentiable_solve(mpc, fields, traj, weights, alpha_k, r)  # r [b, 3 contacts], the record's order: r.grad as well, by one
                                                                           # more launch (hmpc_adjoint_model; csrc/hmpc_model_adjoint.hip)
    forces = differentiable_solve_limits(mpc, fields, traj, weights, alpha_k, mu=mu)  # mu [b], the instances' friction parameter: mu.grad
                                                                                      # as well (hmpc_adjoint_limits; csrc/hmpc_limit_adjoint.hip)
    forces = differentiable_solve_fields(mpc, fields)  # any of p, v, q, w, r, joint_angles, weights, Alpha_K, traj (Rhand, f_max_hand) in
                                                       # ``fields`` a tensor: its .grad, the orientation and the joint angles through the
                                                       # assembly (hmpc_adjoint_record; csrc/hmpc_pose_adjoint.hip)

    jac, grad_params, grad_limits = wrench_jacobian(mpc, step=0)  # behind a solve: d u_step / d record [b, U, record floats], from ONE
                                                                  # multi-seed adjoint launch (hmpc_solve_adjoint_multi;
                                                                  # csrc/hmpc_adjoint_multi.hip) and ONE chain launch behind it
                                                                  # (hmpc_adjoint_chain_multi; csrc/hmpc_adjoint_chain.hip)

The derivatives are those of the QP's solution with its linearisation and the active set frozen (exact wherever the active set is locally
constant).  Records are packed on the host (device-resident packing is a matter of its own); ``grad_x0`` and ``dir`` of the last backward
stay available through ``mpc.download_adjoint()``.  A backward is refused when the ``BatchedMPC`` object has uploaded, solved or been given
other records or outputs since its forward (``BatchedMPC.generation``); calls made on the C handle behind the object's back are not seen."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, records


def _buffers(mpc, device):
    """Caller-owned adjoint buffers of ``mpc`` as torch tensors (made once per handle, for max_batch rows), and the handle pointed at
    them: a ``set_device_adjoint`` of the user's since the last backward is undone here, so that what backward reads is what the launch
    writes."""
    buf = getattr(mpc, "_autograd_buffers", None)
    if buf is None:
        shapes = mpc.result_shapes("adjoint", (mpc.max_batch,))
        buf = {k: torch.zeros(s, dtype=torch.float64, device=device) for k, s in shapes.items()}
        mpc._autograd_buffers = buf
    if mpc.get_device_adjoint() != {k: buf[k].data_ptr() for k in mpc.ADJOINT_KEYS}:
        mpc.set_device_adjoint(*[buf[k].data_ptr() for k in mpc.ADJOINT_KEYS], keepalive=buf)
    return buf


def _model_buffers(mpc, device):
    """The same for the model gradients (``set_device_adjoint_model``)."""
    buf = getattr(mpc, "_autograd_model_buffers", None)
    if buf is None:
        shapes = mpc.result_shapes("adjoint_model", (mpc.max_batch,))
        buf = {k: torch.zeros(s, dtype=torch.float64, device=device) for k, s in shapes.items()}
        mpc._autograd_model_buffers = buf
    if mpc.get_device_adjoint_model() != {k: buf[k].data_ptr() for k in mpc.MODEL_ADJOINT_KEYS}:
        mpc.set_device_adjoint_model(*[buf[k].data_ptr() for k in mpc.MODEL_ADJOINT_KEYS], keepalive=buf)
    return buf


def _limit_buffers(mpc, device):
    """The same for the limit gradients (``set_device_adjoint_limits``)."""
    buf = getattr(mpc, "_autograd_limit_buffers", None)
    if buf is None:
        shapes = mpc.result_shapes("adjoint_limits", (mpc.max_batch,))
        buf = {k: torch.zeros(s, dtype=torch.float64, device=device) for k, s in shapes.items()}
        mpc._autograd_limit_buffers = buf
    if mpc.get_device_adjoint_limits() != {k: buf[k].data_ptr() for k in mpc.LIMIT_ADJOINT_KEYS}:
        mpc.set_device_adjoint_limits(*[buf[k].data_ptr() for k in mpc.LIMIT_ADJOINT_KEYS], keepalive=buf)
    return buf


def _record_buffers(mpc, device):
    """The same for the record gradients (``set_device_adjoint_record``)."""
    buf = getattr(mpc, "_autograd_record_buffers", None)
    if buf is None:
        shapes = mpc.result_shapes("adjoint_record", (mpc.max_batch,))
        buf = {k: torch.zeros(s, dtype=torch.float64, device=device) for k, s in shapes.items()}
        mpc._autograd_record_buffers = buf
    if mpc.get_device_adjoint_record() != {k: buf[k].data_ptr() for k in mpc.RECORD_ADJOINT_KEYS}:
        mpc.set_device_adjoint_record(*[buf[k].data_ptr() for k in mpc.RECORD_ADJOINT_KEYS], keepalive=buf)
    return buf


def _multi_buffers(mpc, device, n_seeds):
    """The same for the multi-seed adjoint (``set_device_adjoint_multi``), with room for ``n_seeds`` slices of max_batch rows."""
    buf = getattr(mpc, "_autograd_multi_buffers", None)
    if buf is None or buf["summary"].shape[0] < n_seeds:
        shapes = mpc.result_shapes("adjoint_multi", (n_seeds, mpc.max_batch))
        buf = {k: torch.zeros(s, dtype=torch.float64, device=device) for k, s in shapes.items()}
        mpc._autograd_multi_buffers = buf
    now = mpc.get_device_adjoint_multi()
    if {k: now[k] for k in mpc.ADJOINT_KEYS} != {k: buf[k].data_ptr() for k in mpc.ADJOINT_KEYS}:
        mpc.set_device_adjoint_multi(buf["summary"].shape[0], *[buf[k].data_ptr() for k in mpc.ADJOINT_KEYS], keepalive=buf)
    return buf


def _chain_buffers(mpc, device, n_seeds):
    """The same for the compact arrays of the multi-seed chain (``set_device_adjoint_chain_multi``); no detail array is asked for."""
    buf = getattr(mpc, "_autograd_chain_buffers", None)
    if buf is None or buf["grad_rpy"].shape[0] < n_seeds:
        shapes = mpc.result_shapes("adjoint_chain_multi", (n_seeds, mpc.max_batch))
        buf = {k: torch.zeros(shapes[k], dtype=torch.float64, device=device) for k in _lib.CHAIN_COMPACT}  # (no detail array)
        mpc._autograd_chain_buffers = buf
    now = mpc.get_device_adjoint_chain_multi()
    want = {k: (buf[k].data_ptr() if k in buf else 0) for k in mpc.CHAIN_KEYS}
    if {k: now[k] for k in mpc.CHAIN_KEYS} != want:
        mpc.set_device_adjoint_chain_multi(buf["grad_rpy"].shape[0], keepalive=buf, **{k + "_ptr": buf[k].data_ptr() for k in buf})
    return buf


def wrench_jacobian(mpc, step=0, generation=None):
    """Behind a solve of ``mpc``: the Jacobian of the wrench of horizon step ``step`` in every float of the packed record, with the
    linearisation and the active set frozen.  The unit seeds e_c at ``step`` go on the device and TWO calls follow on torch's current
    stream into torch-owned buffers: ONE multi-seed launch (hmpc_solve_adjoint_multi) runs the matrix backward pass once for all 6 contacts
    of them, and ONE chain launch (hmpc_adjoint_chain_multi) runs model gradients -> limit gradients -> record gradients of every row
    behind one assembly.  Returns ``(jac, grad_params, grad_limits)``: float64 CUDA tensors [batch, U, NF + 12 h] (``d u_step[c] / d
    record``: row c is what ``differentiable_solve_fields`` returns under grad_output = e_c, bit for bit), [batch, U, 4] and [batch, U, 3 +
    contacts].  The call leaves no selection (``select_adjoint_seed``) behind and moves none of the single-seed adjoint, model, limit and
    record buffers.  With ``generation`` (``mpc.generation`` as it stood behind the solve) the call is refused when the object has
    uploaded, solved or been given other records or outputs since, as a backward of ``differentiable_solve`` is."""
    if generation is not None and mpc.generation != generation:
        raise RuntimeError("wrench_jacobian: the handle has solved another batch since; its forces are gone")
    b, nc, hz = mpc.batch, mpc.contacts, mpc.horizon
    u = 6 * nc
    if not 0 <= step < hz:
        raise ValueError(f"wrench_jacobian: step {step} outside the horizon")
    device = torch.device("cuda", mpc.device)
    _multi_buffers(mpc, device, u)
    cbuf = _chain_buffers(mpc, device, u)
    seeds = torch.zeros((u, b, hz, u), dtype=torch.float64, device=device)
    seeds[torch.arange(u), :, step, torch.arange(u)] = 1.0
    stream = torch.cuda.current_stream(device).cuda_stream
    mpc.solve_adjoint_multi(seeds.data_ptr(), u, stream)
    mpc.adjoint_chain_multi(seeds.data_ptr(), stream)

    def rows(key):  # slices [u][batch][...] of the current batch -> [batch, u, ...]: one transposing copy
        flat = cbuf[key].reshape(-1)
        n = flat.numel() // (cbuf[key].shape[0] * mpc.max_batch)
        return flat[:u * b * n].reshape(u, b, n).transpose(0, 1).contiguous()

    return rows("grad_record"), rows("grad_params"), rows("grad_limits")


FIELD_NAMES = ("p", "v", "q", "w", "r", "joint_angles", "weights", "Alpha_K", "traj", "Rhand", "f_max_hand")


class _SolveFields(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mpc, fields, names, *tensors):
        f = dict(fields)
        for name, t in zip(names, tensors):
            f[name] = t.detach().cpu().numpy()
        device = torch.device("cuda", mpc.device)
        mpc.upload(records.pack_records(f, mpc.horizon, mpc.contacts))
        mpc.solve(torch.cuda.current_stream(device).cuda_stream)
        forces, _ = mpc.download()  # (the safe pass: repaired forces, in the handle's force buffer as well)
        ctx.mpc, ctx.generation, ctx.device, ctx.names = mpc, mpc.generation, device, names
        ctx.meta = [(t.shape, t.dtype, t.device) for t in tensors]
        return torch.from_numpy(np.ascontiguousarray(forces)).to(device)

    @staticmethod
    def backward(ctx, grad_output):
        mpc = ctx.mpc
        if mpc.generation != ctx.generation:
            raise RuntimeError("differentiable_solve_fields: the handle has solved another batch since this forward; its forces are gone")
        b, nc, hz = mpc.batch, mpc.contacts, mpc.horizon
        _buffers(mpc, ctx.device), _model_buffers(mpc, ctx.device), _limit_buffers(mpc, ctx.device)  # (before the adjoint, as in _Solve)
        rbuf = _record_buffers(mpc, ctx.device)
        seed = grad_output.detach().to(device=ctx.device, dtype=torch.float64).contiguous()
        stream = torch.cuda.current_stream(ctx.device).cuda_stream
        mpc.solve_adjoint(seed.data_ptr(), stream)
        mpc.adjoint_model(stream)
        mpc.adjoint_limits(seed.data_ptr(), stream)
        mpc.adjoint_record(stream)
        _, off, length = records._layout(nc)
        grads = []
        for name, (shape, dtype, dev), need in zip(ctx.names, ctx.meta, ctx.needs_input_grad[3:]):
            n = 12 * hz if name == "traj" else length[name]
            grads.append(rbuf["grad_record"][:b, off[name]:off[name] + n].to(device=dev, dtype=dtype, copy=True).reshape(shape) if need else None)
        return (None, None, None) + tuple(grads)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mpc, fields, traj, weights, alpha_k, r=None, mu=None):
        f = dict(fields)
        if r is not None:
            f["r"] = r.detach().cpu().numpy()
        f["traj"] = traj.detach().cpu().numpy()
        f["weights"] = weights.detach().cpu().numpy()
        f["Alpha_K"] = alpha_k.detach().cpu().numpy()
        device = torch.device("cuda", mpc.device)
        stream = torch.cuda.current_stream(device).cuda_stream
        if mu is not None:  # (a float32 CUDA tensor of the handle's own; it stays set on the handle)
            mu32 = mu.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous().clone()
            mpc.set_instance_mu(mu32.data_ptr(), keepalive=mu32)
        mpc.upload(records.pack_records(f, mpc.horizon, mpc.contacts))
        mpc.solve(stream)
        forces, _ = mpc.download()  # (the safe pass: repaired forces, in the handle's force buffer as well)
        ctx.mpc, ctx.generation, ctx.device = mpc, mpc.generation, device  # (after the download: the safe pass replaces no batch)
        ctx.meta = [(t.shape, t.dtype, t.device) for t in (traj, weights, alpha_k)]
        ctx.r_meta = None if r is None else (r.shape, r.dtype, r.device)
        ctx.mu_meta = None if mu is None else (mu.shape, mu.dtype, mu.device)
        return torch.from_numpy(np.ascontiguousarray(forces)).to(device)

    @staticmethod
    def backward(ctx, grad_output):
        mpc = ctx.mpc
        if mpc.generation != ctx.generation:  # an upload, a solve, new records or outputs through this object since the forward
            raise RuntimeError("differentiable_solve: the handle has solved another batch since this forward; its forces are gone")
        b = mpc.batch
        buf = _buffers(mpc, ctx.device)
        want_r = ctx.r_meta is not None and ctx.needs_input_grad[5]
        mbuf = _model_buffers(mpc, ctx.device) if want_r else None  # (before the adjoint: moving buffers makes nothing of it stale)
        want_mu = ctx.mu_meta is not None and ctx.needs_input_grad[6]
        lbuf = _limit_buffers(mpc, ctx.device) if want_mu else None
        seed = grad_output.detach().to(device=ctx.device, dtype=torch.float64).contiguous()
        mpc.solve_adjoint(seed.data_ptr(), torch.cuda.current_stream(ctx.device).cuda_stream)
        grads = []
        for key, (shape, dtype, dev), need in zip(("grad_traj", "grad_weights", "grad_alpha"), ctx.meta, ctx.needs_input_grad[2:]):
            # (a copy in every case: a float64 leaf on the handle's device would otherwise get a view of the handle's own buffer as
            #  its .grad, which the next launch overwrites)
            grads.append(buf[key][:b].to(device=dev, dtype=dtype, copy=True).reshape(shape) if need else None)
        grad_r = None
        if want_r:
            mpc.adjoint_model(torch.cuda.current_stream(ctx.device).cuda_stream)
            shape, dtype, dev = ctx.r_meta
            grad_r = mbuf["grad_r"][:b].to(device=dev, dtype=dtype, copy=True).reshape(shape)
        grad_mu = None
        if want_mu:
            mpc.adjoint_limits(seed.data_ptr(), torch.cuda.current_stream(ctx.device).cuda_stream)
            shape, dtype, dev = ctx.mu_meta
            grad_mu = lbuf["grad_limits"][:b, 0].to(device=dev, dtype=dtype, copy=True).reshape(shape)
        if ctx.mu_meta is not None:
            return (None, None) + tuple(grads) + (grad_r, grad_mu)
        return (None, None) + tuple(grads) + ((grad_r,) if ctx.r_meta is not None else ())


def differentiable_solve(mpc, fields, traj, weights, alpha_k, r=None):
    """Solves the batch ``fields`` (the dict ``records.pack_records`` takes) with its reference trajectory, tracking weights and Alpha_K
    replaced by the tensors ``traj`` [b, 12 h], ``weights`` [b, 12] and ``alpha_k`` [b, 6 contacts] (any device, any float dtype), and returns
    the forces as a CUDA float32 tensor [b, h * 6 contacts] that autograd differentiates in those three.  With a tensor ``r`` [b, 3 contacts]
    (the record's order: axis, then contact) the foot positions are replaced as well and the backward returns their gradient too, by one
    more launch behind the adjoint (hmpc_adjoint_model); with ``r=None`` nothing is launched beyond the adjoint."""
    if r is None:
        return _Solve.apply(mpc, fields, traj, weights, alpha_k)
    return _Solve.apply(mpc, fields, traj, weights, alpha_k, r)


def differentiable_solve_limits(mpc, fields, traj, weights, alpha_k, r=None, mu=None):
    """``differentiable_solve`` with the instances' friction parameter as one more input (its own entry point: the older function keeps
    its parameter list).  With a tensor ``mu`` [b] the instances solve under their own friction parameter (``set_instance_mu`` with a
    float32 CUDA copy, which STAYS SET on the handle after the call: later solves of ``mpc`` use it until ``mpc.set_instance_mu(0)``),
    and the backward returns its gradient too, by one more launch behind the adjoint (hmpc_adjoint_limits); with ``mu=None`` this is
    ``differentiable_solve``: the same launches, every bit of the other gradients the same."""
    if mu is None:
        return differentiable_solve(mpc, fields, traj, weights, alpha_k, r)
    return _Solve.apply(mpc, fields, traj, weights, alpha_k, r, mu)


def differentiable_solve_fields(mpc, fields):
    """Solves the batch ``fields`` (the dict ``records.pack_records`` takes), any of whose entries ``p, v, q, w, r, joint_angles, weights,
    Alpha_K, traj`` (and ``Rhand, f_max_hand`` for three contacts) may be a torch tensor (any device, any float dtype, the shape
    ``pack_records`` takes with a leading batch dimension); the rest are arrays.  Returns the forces as a CUDA float32 tensor [b, h * 6
    contacts] that autograd differentiates in every tensor given: the backward enqueues adjoint -> model gradients -> limit gradients ->
    record gradients on torch's current stream into torch-owned buffers and returns, for each tensor that needs it, a copy of its slice
    of ``grad_record``.  The gradient in ``q`` is the total one -- through the Euler angles of the state, Acd, Bcd and the constraint
    block -- of the quaternion as given (no normalisation is differentiated)."""
    names = tuple(k for k in FIELD_NAMES if k in fields and isinstance(fields[k], torch.Tensor))
    extra = [k for k, v in fields.items() if isinstance(v, torch.Tensor) and k not in names]
    if extra:
        raise ValueError(f"differentiable_solve_fields: no gradient is defined in {extra}")
    return _SolveFields.apply(mpc, fields, names, *[fields[k] for k in names])
