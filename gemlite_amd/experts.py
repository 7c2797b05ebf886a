"""GemLiteExperts: the experts of a mixture-of-experts layer as ONE decode launch whose expert ids are read on the GPU.

``layer(x)`` bakes a layer's weight pointers into the graph node at capture time; which experts a token uses is the router's top-k, a
device tensor known only when the graph replays.  ``GemLiteExperts`` stacks E identical A16W4 layers into one ``[E, K/8, N]`` weight
tensor (scales / zeros ``[E, K/g, N]``, bias ``[E, N]``) and runs ``gemlite_hip_forward_experts`` (include/gemlite_hip.h): slot ``s`` of the
``expert_ids`` tensor is one M = 1 GEMV of expert ``expert_ids[s]``, bit-identical to that expert's own decode launch; the id is loaded
by the kernel, so the call can be captured once and replayed with other ids.  An id outside ``[0, E)`` (-1: "not on this rank") gives a
row of zeros.  Domain: DESIGN.md §3.1.3 — 4-bit weights in 32-bit words, fp16 / bf16, grouped scales / zeros, N % 16 == 0, K % 256 == 0.
There is no slow path: layers outside the domain are refused by ``from_layers``.

``GemLiteExpertsMLP`` runs a whole expert MLP in two such launches (``gemlite_hip_forward_experts_fused``):
``gate_up.forward_glu`` stores ``silu(gate) * up`` of experts stacked ``[gate; up]`` along N, ``down.forward_combine`` stores the
routing-weight sum over a token's slots.  Every member is rounded as its slot of ``forward``; the epilogues run in fp32 on those values.

Batches: ``experts.route(ids)`` sorts the slots by expert on the GPU into work blocks (an ``ExpertsRouting``) and
``experts.forward_batched(x, ids, routing)`` streams every expert's weights once per work block through the MFMA rows kernel
(``gemlite_hip_experts_route`` / ``gemlite_hip_forward_experts_rows``).  Opt-in: ``forward`` never dispatches to it.

The batched MLP in four launches: ``experts.forward_batched_glu`` is the rows launch with SwiGLU in its epilogue
(``gemlite_hip_forward_experts_rows_glu``), ``experts.combine_batched`` the routing-weight sum over a token's slots in one launch
(``gemlite_hip_experts_combine``), ``GemLiteExpertsMLP.forward_batched_fused`` route + GLU + down + combine.  Opt-in as well.

The router's top-k: ``experts_topk(logits, top_k, ...)`` / ``ExpertsRouter`` turn router logits into the ``topk_ids`` and
``topk_weights`` all of the above begin with, in one launch (``gemlite_hip_experts_topk``); ``GemLiteExpertsMLP.forward_routed`` and
``forward_batched_fused_routed`` put it in front of the MLP.  Opt-in as well.
"""
import threading
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _hip
from . import core
from .dtypes import DTYPE_TO_TORCH, TORCH_TO_DTYPE, DType

MAX_SLOTS = 65535  # of one launch (grid.y)

_TEMPLATES: dict = {}
_TEMPLATES_LOCK = threading.Lock()


def _first(t: Tensor) -> Tensor:
    """Expert 0's slice of a stacked tensor (absent metadata and a scalar zero are not stacked)."""
    return t[0] if t.dim() == 3 else t


def _build_template(W_q: Tensor, scales: Tensor, zeros: Tensor, bias: Optional[Tensor], meta_args) -> bytes:
    """The static half of a gemlite_hip_experts_args: expert 0 as a layer (core._build_template), the expert count and strides."""
    e = _hip.ExpertsArgs()
    e.struct_size = _hip.C.sizeof(_hip.ExpertsArgs)
    e.layer = _hip.ForwardArgs.from_buffer_copy(core._build_template(_first(W_q), _first(scales), _first(zeros), meta_args))
    e.layer.M = 1
    e.layer.stride_xk, e.layer.stride_om, e.layer.stride_on = 1, W_q.shape[2], 1
    e.n_experts = W_q.shape[0]
    e.stride_expert_w = W_q.stride(0) * W_q.element_size()
    meta = scales if scales.dim() == 3 else (zeros if zeros.dim() == 3 else None)
    e.stride_expert_meta = 0 if meta is None else meta.stride(0) * meta.element_size()
    if bias is not None:
        e.bias = bias.data_ptr()
        e.stride_expert_bias = bias.stride(0) * bias.element_size()
    return bytes(e)


def _static_args(W_q: Tensor, scales: Tensor, zeros: Tensor, bias: Optional[Tensor], meta_args) -> "_hip.ExpertsArgs":
    """A FRESH gemlite_hip_experts_args with the static fields filled in; the image is cached per everything it is derived from."""
    key = core._template_key(W_q, scales, zeros, meta_args) + (
        (None,) if bias is None else (bias.data_ptr(), tuple(bias.shape), bias.stride(), bias.dtype))
    t = _TEMPLATES.get(key)
    if t is None:
        t = _build_template(W_q, scales, zeros, bias, meta_args)
        with _TEMPLATES_LOCK:
            while len(_TEMPLATES) >= 1024:
                _TEMPLATES.pop(next(iter(_TEMPLATES)), None)
            _TEMPLATES[key] = t
    return _hip.ExpertsArgs.from_buffer_copy(t)


def _call_args(x2: Tensor, ids: Tensor, out_ptr: int, bias: Optional[Tensor], tensor_args, meta_args, slots_per_x_row: int):
    W_q, scales, zeros = tensor_args
    e = _static_args(W_q, scales, zeros, bias, meta_args)
    e.layer.x, e.layer.out = x2.data_ptr(), out_ptr
    e.layer.input_dtype = TORCH_TO_DTYPE[x2.dtype].value
    e.layer.stride_xm = x2.stride(0)
    e.ids = ids.data_ptr()
    e.ids_dtype = TORCH_TO_DTYPE[ids.dtype].value
    e.n_slots = ids.numel()
    e.slots_per_x_row = slots_per_x_row
    e.stride_x_row = x2.stride(0)
    e.stride_out_slot = W_q.shape[2]
    return e


def _split(x: Tensor, expert_ids: Tensor, K: int):
    """-> (rows of x, slots per row of x): x [..., K] is one row per token, shared by its top_k slots; x [..., top_k, K] one row per slot."""
    if expert_ids.dim() < 1:
        raise ValueError("expert_ids should be [..., top_k]")
    lead, top_k = tuple(expert_ids.shape[:-1]), expert_ids.shape[-1]
    if tuple(x.shape) == lead + (K,):
        return expert_ids.numel() // max(top_k, 1), top_k
    if tuple(x.shape) == lead + (top_k, K):
        return expert_ids.numel(), 1
    raise ValueError(f"x is {tuple(x.shape)}; expert_ids {tuple(expert_ids.shape)} asks for {lead + (K,)} or {lead + (top_k, K)}")


def _forward_impl(x: Tensor, expert_ids: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    W_q = tensor_args[0]
    N, K = W_q.shape[2], W_q.shape[1] * meta_args[4]
    lib = _hip.load()
    for t, name in ((x, "x"), (expert_ids, "expert_ids"), (W_q, "W_q")):
        _hip.require_gpu_tensor(t, name)
    if x.device != W_q.device or expert_ids.device != W_q.device:
        raise _hip.GemliteHipError(f"x is on {x.device}, expert_ids on {expert_ids.device}, the packed weights on {W_q.device}")
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    rows, spx = _split(x, expert_ids, K)
    out = torch.empty(tuple(expert_ids.shape) + (N,), dtype=x.dtype, device=x.device)
    if expert_ids.numel() == 0:
        return out
    x2 = x.contiguous().view(rows, K)
    ids = expert_ids.contiguous()
    e = _call_args(x2, ids, out.data_ptr(), bias, tensor_args, meta_args, spx)
    with _hip.on_device(x.device):  # launches go to the tensor's device and torch's current stream there
        rc = lib.gemlite_hip_forward_experts(_hip.C.byref(e), _hip.current_stream_handle(x.device))
    _hip.raise_for_status(rc, "gemlite_hip_forward_experts")
    return out


@torch.library.custom_op("gemlite::forward_experts", mutates_args=())
def forward_experts(x: Tensor, expert_ids: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    return _forward_impl(x, expert_ids, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::forward_experts")
def _forward_experts_fake(x, expert_ids, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    _split(x, expert_ids, W_q.shape[1] * meta_args[4])
    return torch.empty(tuple(expert_ids.shape) + (W_q.shape[2],), device=x.device, dtype=x.dtype)


# ---- the fused epilogues (gemlite_hip_forward_experts_fused): GLU on the gate/up launch, the routing-weight combine on the down launch ----
def _fused_args(e: "_hip.ExpertsArgs", epilogue: int, weights_ptr: int = 0, weights_dtype: int = 0, slots_per_token: int = 0):
    f = _hip.ExpertsFusedArgs()
    f.struct_size = _hip.C.sizeof(_hip.ExpertsFusedArgs)
    f.epilogue = epilogue
    f.experts = e
    f.activation = _hip.ACT_SILU
    f.weights_dtype = weights_dtype
    f.weights = weights_ptr or None
    f.slots_per_token = slots_per_token
    return f


def _weights_like(weights: Tensor, expert_ids: Tensor, x: Tensor):
    if tuple(weights.shape) != tuple(expert_ids.shape):
        raise ValueError(f"weights are {tuple(weights.shape)}, expert_ids {tuple(expert_ids.shape)}: one weight per slot")
    if weights.dtype not in (torch.float32, x.dtype):
        raise NotImplementedError(f"weights are {weights.dtype}: float32 or {x.dtype}")


def _fused_impl(epilogue: int, x: Tensor, expert_ids: Tensor, weights: Optional[Tensor], bias: Optional[Tensor],
                tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    W_q = tensor_args[0]
    N, K = W_q.shape[2], W_q.shape[1] * meta_args[4]
    glu = epilogue == _hip.EXPERTS_GLU
    lib = _hip.load()
    tensors = ((x, "x"), (expert_ids, "expert_ids"), (W_q, "W_q")) + (() if glu else ((weights, "weights"),))
    for t, name in tensors:
        _hip.require_gpu_tensor(t, name)
    if any(t.device != W_q.device for t, _ in tensors):
        raise _hip.GemliteHipError("x, expert_ids, weights and the packed weights live on different devices: "
                                   + ", ".join(f"{name} on {t.device}" for t, name in tensors))
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    rows, spx = _split(x, expert_ids, K)
    if glu:
        width = N // 2
        out = torch.empty(tuple(expert_ids.shape) + (width,), dtype=x.dtype, device=x.device)
    else:
        _weights_like(weights, expert_ids, x)
        width = N
        out = torch.empty(tuple(expert_ids.shape[:-1]) + (width,), dtype=x.dtype, device=x.device)
    if expert_ids.numel() == 0:
        return out.zero_()  # (COMBINE with top_k = 0: a sum without terms)
    x2 = x.contiguous().view(rows, K)
    ids = expert_ids.contiguous()
    e = _call_args(x2, ids, out.data_ptr(), bias, tensor_args, meta_args, spx)
    e.stride_out_slot = width
    if glu:
        f = _fused_args(e, epilogue)
    else:
        w = weights.contiguous()
        f = _fused_args(e, epilogue, w.data_ptr(), TORCH_TO_DTYPE[w.dtype].value, expert_ids.shape[-1])
    with _hip.on_device(x.device):
        rc = lib.gemlite_hip_forward_experts_fused(_hip.C.byref(f), _hip.current_stream_handle(x.device))
    _hip.raise_for_status(rc, "gemlite_hip_forward_experts_fused")
    return out


@torch.library.custom_op("gemlite::forward_experts_glu", mutates_args=())
def forward_experts_glu(x: Tensor, expert_ids: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    return _fused_impl(_hip.EXPERTS_GLU, x, expert_ids, None, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::forward_experts_glu")
def _forward_experts_glu_fake(x, expert_ids, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    _split(x, expert_ids, W_q.shape[1] * meta_args[4])
    return torch.empty(tuple(expert_ids.shape) + (W_q.shape[2] // 2,), device=x.device, dtype=x.dtype)


@torch.library.custom_op("gemlite::forward_experts_combine", mutates_args=())
def forward_experts_combine(x: Tensor, expert_ids: Tensor, weights: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor],
                            meta_args: List[int]) -> Tensor:
    return _fused_impl(_hip.EXPERTS_COMBINE, x, expert_ids, weights, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::forward_experts_combine")
def _forward_experts_combine_fake(x, expert_ids, weights, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    _split(x, expert_ids, W_q.shape[1] * meta_args[4])
    _weights_like(weights, expert_ids, x)
    return torch.empty(tuple(expert_ids.shape[:-1]) + (W_q.shape[2],), device=x.device, dtype=x.dtype)


# ---- batches (gemlite_hip_experts_route + gemlite_hip_forward_experts_rows): the slots are sorted by expert on the GPU
# and every expert's weights stream once per work block of up to R slots through the MFMA rows kernel ----
ROWS_PER_BLOCK = (16, 32, 48, 64)
ROWS_DOMAIN = ("domain: rows_per_block 16 / 32 / 48 / 64 (groups of 32: 16 / 32), at most %d experts and %d slots, 4-byte aligned outputs, "
               "all of x below 2^31 bytes" % (_hip.EXPERTS_ROWS_MAX_EXPERTS, MAX_SLOTS))


def rows_blocks_max(n_slots: int, n_experts: int, rows_per_block: int) -> int:
    """Bmax of the header: the work blocks a routing can need, which is grid.y of the rows launch."""
    return -(-n_slots // rows_per_block) + min(n_experts + 1, n_slots)


def rows_workspace_ints(n_slots: int, n_experts: int, rows_per_block: int) -> int:
    """int32 entries of the work table: 4 of header, block_expert[Bmax], block_rows[Bmax * R] (gemlite_hip_experts_rows_workspace_bytes / 4)."""
    b = rows_blocks_max(n_slots, n_experts, rows_per_block)
    return 4 + b + b * rows_per_block


def _rows_args(e: "_hip.ExpertsArgs", rows_per_block: int, workspace: Optional[Tensor]) -> "_hip.ExpertsRowsArgs":
    r = _hip.ExpertsRowsArgs()
    r.struct_size = _hip.C.sizeof(_hip.ExpertsRowsArgs)
    r.rows_per_block = int(rows_per_block)
    r.experts = e
    if workspace is not None:
        r.workspace = workspace.data_ptr()
        r.workspace_bytes = workspace.numel() * workspace.element_size()
    return r


def _stand_in_args(bias: Optional[Tensor], tensor_args, meta_args, n_slots: int) -> "_hip.ExpertsArgs":
    """A request with stand-ins for x / out / ids (one row per slot): what the host-only queries are asked with."""
    W_q, scales, zeros = tensor_args
    e = _static_args(W_q, scales, zeros, bias, meta_args)
    e.layer.x = e.layer.out = e.ids = 0x1000
    e.layer.stride_xm = e.stride_x_row = e.layer.K
    e.ids_dtype = DType.INT32.value
    e.n_slots, e.slots_per_x_row = max(int(n_slots), 1), 1
    e.stride_out_slot = e.layer.N
    return e


def _raise_rows(rc: int, what: str):
    if rc in (_hip.ERR_BAD_SHAPE, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_ARGUMENT, _hip.ERR_WORKSPACE):
        raise NotImplementedError(f"{what}: {_hip.status_string(rc)} ({ROWS_DOMAIN})")
    _hip.raise_for_status(rc, what)


def _resolve_rows(bias: Optional[Tensor], tensor_args, meta_args, n_slots: int, rows_per_block: Optional[int]) -> int:
    """The R the library resolves for these experts and this many slots (host only); refusals in words."""
    want = 0 if rows_per_block is None else int(rows_per_block)
    if want and want not in ROWS_PER_BLOCK:
        raise ValueError(f"rows_per_block is {rows_per_block}: one of {ROWS_PER_BLOCK}, or None for the library's default")
    if want > 32 and meta_args[2] == 32:
        raise NotImplementedError(f"rows_per_block is {want}: groups of 32 take 16 or 32 rows per work block (the registers of the kernel)")
    r = _rows_args(_stand_in_args(bias, tensor_args, meta_args, n_slots), want, None)
    rc = _hip.load().gemlite_hip_experts_rows_per_block(_hip.C.byref(r))
    if rc < 0:
        _raise_rows(rc, f"GemLiteExperts.route: {n_slots} slots over {tensor_args[0].shape[0]} experts, rows_per_block={rows_per_block}")
    return rc


def _route_impl(expert_ids: Tensor, rows_per_block: int, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    W_q = tensor_args[0]
    lib = _hip.load()
    for t, name in ((expert_ids, "expert_ids"), (W_q, "W_q")):
        _hip.require_gpu_tensor(t, name)
    if expert_ids.device != W_q.device:
        raise _hip.GemliteHipError(f"expert_ids are on {expert_ids.device}, the packed weights on {W_q.device}")
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    n_slots = expert_ids.numel()
    ws = torch.empty(rows_workspace_ints(max(n_slots, 1), W_q.shape[0], rows_per_block), dtype=torch.int32, device=W_q.device)
    if n_slots == 0:
        return ws.zero_()  # (no work block is used)
    ids = expert_ids.contiguous()
    e = _stand_in_args(bias, tensor_args, meta_args, n_slots)
    e.ids, e.ids_dtype = ids.data_ptr(), TORCH_TO_DTYPE[ids.dtype].value
    r = _rows_args(e, rows_per_block, ws)
    with _hip.on_device(W_q.device):
        rc = lib.gemlite_hip_experts_route(_hip.C.byref(r), _hip.current_stream_handle(W_q.device))
    if rc != _hip.OK:
        _raise_rows(rc, "gemlite_hip_experts_route")
    return ws


def _forward_rows_impl(x: Tensor, expert_ids: Tensor, workspace: Tensor, rows_per_block: int, bias: Optional[Tensor],
                       tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    W_q = tensor_args[0]
    N, K = W_q.shape[2], W_q.shape[1] * meta_args[4]
    lib = _hip.load()
    for t, name in ((x, "x"), (expert_ids, "expert_ids"), (workspace, "workspace"), (W_q, "W_q")):
        _hip.require_gpu_tensor(t, name)
    if x.device != W_q.device or expert_ids.device != W_q.device or workspace.device != W_q.device:
        raise _hip.GemliteHipError(f"x is on {x.device}, expert_ids on {expert_ids.device}, the routing on {workspace.device}, "
                                   f"the packed weights on {W_q.device}")
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    rows, spx = _split(x, expert_ids, K)
    out = torch.empty(tuple(expert_ids.shape) + (N,), dtype=x.dtype, device=x.device)
    if expert_ids.numel() == 0:
        return out
    if workspace.dtype != torch.int32 or not workspace.is_contiguous():
        raise ValueError(f"the routing workspace is {workspace.dtype}, contiguous={workspace.is_contiguous()}: a contiguous int32 tensor")
    x2 = x.contiguous().view(rows, K)
    ids = expert_ids.contiguous()
    r = _rows_args(_call_args(x2, ids, out.data_ptr(), bias, tensor_args, meta_args, spx), rows_per_block, workspace)
    with _hip.on_device(x.device):
        rc = lib.gemlite_hip_forward_experts_rows(_hip.C.byref(r), _hip.current_stream_handle(x.device))
    if rc != _hip.OK:
        _raise_rows(rc, "gemlite_hip_forward_experts_rows")
    return out


@torch.library.custom_op("gemlite::experts_route", mutates_args=())
def experts_route(expert_ids: Tensor, rows_per_block: int, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    return _route_impl(expert_ids, rows_per_block, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::experts_route")
def _experts_route_fake(expert_ids, rows_per_block, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    return torch.empty(rows_workspace_ints(max(expert_ids.numel(), 1), W_q.shape[0], rows_per_block), device=W_q.device, dtype=torch.int32)


@torch.library.custom_op("gemlite::forward_experts_rows", mutates_args=())
def forward_experts_rows(x: Tensor, expert_ids: Tensor, workspace: Tensor, rows_per_block: int, bias: Optional[Tensor],
                         tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    return _forward_rows_impl(x, expert_ids, workspace, rows_per_block, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::forward_experts_rows")
def _forward_experts_rows_fake(x, expert_ids, workspace, rows_per_block, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    _split(x, expert_ids, W_q.shape[1] * meta_args[4])
    return torch.empty(tuple(expert_ids.shape) + (W_q.shape[2],), device=x.device, dtype=x.dtype)


# ---- the batched MLP without an fp32 intermediate: SwiGLU inside the gate/up rows launch, the combine in one launch ----
GLU_ROWS_DOMAIN = ("domain: N % 32 == 0 ([gate; up] halves in whole 16-column tiles), groups of 64 or more (groups of 32 have no GLU form), "
                   "rows_per_block up to 64 for groups >= 128 and up to 32 for groups of 64")
COMBINE_DOMAIN = ("domain: fp16 / bf16 y with N %% 16 == 0, 1 <= top_k <= %d, at most %d slots, 4-byte aligned rows with even strides"
                  % (_hip.EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN, MAX_SLOTS))


def _glu_rows_args(r: "_hip.ExpertsRowsArgs") -> "_hip.ExpertsRowsGluArgs":
    g = _hip.ExpertsRowsGluArgs()
    g.struct_size = _hip.C.sizeof(_hip.ExpertsRowsGluArgs)
    g.activation = _hip.ACT_SILU
    g.rows = r
    return g


def _raise_glu_rows(rc: int, what: str):
    if rc in (_hip.ERR_BAD_SHAPE, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_ARGUMENT, _hip.ERR_WORKSPACE):
        raise NotImplementedError(f"{what}: {_hip.status_string(rc)} ({GLU_ROWS_DOMAIN}; {ROWS_DOMAIN})")
    _hip.raise_for_status(rc, what)


def _resolve_rows_glu(bias: Optional[Tensor], tensor_args, meta_args, n_slots: int, rows_per_block: Optional[int]) -> int:
    """_resolve_rows for the GLU launch: the R gemlite_hip_experts_rows_glu_per_block resolves (host only); refusals in words."""
    want = 0 if rows_per_block is None else int(rows_per_block)
    if want and want not in ROWS_PER_BLOCK:
        raise ValueError(f"rows_per_block is {rows_per_block}: one of {ROWS_PER_BLOCK}, or None for the library's default")
    g = _glu_rows_args(_rows_args(_stand_in_args(bias, tensor_args, meta_args, n_slots), want, None))
    rc = _hip.load().gemlite_hip_experts_rows_glu_per_block(_hip.C.byref(g))
    if rc < 0:
        _raise_glu_rows(rc, f"GemLiteExperts.forward_batched_glu: N={tensor_args[0].shape[2]}, groups of {meta_args[2]}, {n_slots} slots over "
                            f"{tensor_args[0].shape[0]} experts, rows_per_block={rows_per_block}")
    return rc


def _forward_rows_glu_impl(x: Tensor, expert_ids: Tensor, workspace: Tensor, rows_per_block: int, bias: Optional[Tensor],
                           tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    W_q = tensor_args[0]
    N, K = W_q.shape[2], W_q.shape[1] * meta_args[4]
    lib = _hip.load()
    for t, name in ((x, "x"), (expert_ids, "expert_ids"), (workspace, "workspace"), (W_q, "W_q")):
        _hip.require_gpu_tensor(t, name)
    if x.device != W_q.device or expert_ids.device != W_q.device or workspace.device != W_q.device:
        raise _hip.GemliteHipError(f"x is on {x.device}, expert_ids on {expert_ids.device}, the routing on {workspace.device}, "
                                   f"the packed weights on {W_q.device}")
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    rows, spx = _split(x, expert_ids, K)
    out = torch.empty(tuple(expert_ids.shape) + (N // 2,), dtype=x.dtype, device=x.device)
    if expert_ids.numel() == 0:
        return out
    if workspace.dtype != torch.int32 or not workspace.is_contiguous():
        raise ValueError(f"the routing workspace is {workspace.dtype}, contiguous={workspace.is_contiguous()}: a contiguous int32 tensor")
    x2 = x.contiguous().view(rows, K)
    ids = expert_ids.contiguous()
    e = _call_args(x2, ids, out.data_ptr(), bias, tensor_args, meta_args, spx)
    e.stride_out_slot = N // 2
    g = _glu_rows_args(_rows_args(e, rows_per_block, workspace))
    with _hip.on_device(x.device):
        rc = lib.gemlite_hip_forward_experts_rows_glu(_hip.C.byref(g), _hip.current_stream_handle(x.device))
    if rc != _hip.OK:
        _raise_glu_rows(rc, "gemlite_hip_forward_experts_rows_glu")
    return out


def _combine_args(y2: Tensor, ids: Tensor, w: Tensor, out2: Tensor, n_experts: int, top_k: int) -> "_hip.ExpertsCombineArgs":
    """y2 [slots, N] and out2 [tokens, N] with unit inner strides; ids and w contiguous, one entry per slot."""
    c = _hip.ExpertsCombineArgs()
    c.struct_size = _hip.C.sizeof(_hip.ExpertsCombineArgs)
    c.dtype = TORCH_TO_DTYPE[y2.dtype].value
    c.ids_dtype = TORCH_TO_DTYPE[ids.dtype].value
    c.weights_dtype = TORCH_TO_DTYPE[w.dtype].value
    c.y, c.ids, c.weights, c.out = y2.data_ptr(), ids.data_ptr(), w.data_ptr(), out2.data_ptr()
    c.n_slots, c.n_experts, c.slots_per_token, c.N = y2.shape[0], n_experts, top_k, y2.shape[1]
    c.stride_y_slot, c.stride_out_token = y2.stride(0), out2.stride(0)
    return c


def _rows_of(y: Tensor) -> Tensor:
    """[..., N] -> [rows, N] with a unit inner stride and one row stride, as a VIEW where the layout allows (a sliced output of
    forward_batched stays in place), else a copy."""
    N = y.shape[-1]
    if y.dim() >= 1 and y.stride(-1) == 1:
        try:
            return y.view(-1, N)
        except RuntimeError:
            pass
    return y.reshape(-1, N).contiguous()


def _combine_impl(y: Tensor, expert_ids: Tensor, weights: Tensor, n_experts: int) -> Tensor:
    lib = _hip.load()
    _combine_check(y, expert_ids, weights)
    tensors = ((y, "y"), (expert_ids, "expert_ids"), (weights, "weights"))
    for t, name in tensors:
        _hip.require_gpu_tensor(t, name)
    if any(t.device != y.device for t, _ in tensors):
        raise _hip.GemliteHipError("y, expert_ids and weights live on different devices: " + ", ".join(f"{name} on {t.device}" for t, name in tensors))
    N, top_k = y.shape[-1], expert_ids.shape[-1]
    out = torch.empty(tuple(expert_ids.shape[:-1]) + (N,), dtype=y.dtype, device=y.device)
    if out.numel() == 0:
        return out
    if top_k == 0:
        return out.zero_()  # (a sum without terms)
    y2 = _rows_of(y)
    if y2.data_ptr() % 4 or y2.stride(0) % 2:
        y2 = y2.contiguous()
    c = _combine_args(y2, expert_ids.contiguous(), weights.contiguous(), out.view(-1, N), n_experts, top_k)
    with _hip.on_device(y.device):
        rc = lib.gemlite_hip_experts_combine(_hip.C.byref(c), _hip.current_stream_handle(y.device))
    if rc in (_hip.ERR_BAD_SHAPE, _hip.ERR_UNSUPPORTED):
        raise NotImplementedError(f"gemlite_hip_experts_combine: y {tuple(y.shape)}, top_k={top_k}: {_hip.status_string(rc)} ({COMBINE_DOMAIN})")
    _hip.raise_for_status(rc, "gemlite_hip_experts_combine")
    return out


def _combine_check(y: Tensor, expert_ids: Tensor, weights: Tensor):
    if expert_ids.dim() < 1:
        raise ValueError("expert_ids should be [..., top_k]")
    if y.dim() < 2 or tuple(y.shape[:-1]) != tuple(expert_ids.shape):
        raise ValueError(f"y is {tuple(y.shape)}; expert_ids {tuple(expert_ids.shape)} asks for {tuple(expert_ids.shape) + ('N',)}")
    if y.dtype not in (torch.float16, torch.bfloat16):
        raise NotImplementedError(f"y is {y.dtype}: float16 or bfloat16")
    if expert_ids.dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"expert_ids are {expert_ids.dtype}: int32 or int64")
    _weights_like(weights, expert_ids, y)


@torch.library.custom_op("gemlite::forward_experts_rows_glu", mutates_args=())
def forward_experts_rows_glu(x: Tensor, expert_ids: Tensor, workspace: Tensor, rows_per_block: int, bias: Optional[Tensor],
                             tensor_args: List[Tensor], meta_args: List[int]) -> Tensor:
    return _forward_rows_glu_impl(x, expert_ids, workspace, rows_per_block, bias, tensor_args, meta_args)


@torch.library.register_fake("gemlite::forward_experts_rows_glu")
def _forward_experts_rows_glu_fake(x, expert_ids, workspace, rows_per_block, bias, tensor_args, meta_args):
    W_q = tensor_args[0]
    _split(x, expert_ids, W_q.shape[1] * meta_args[4])
    return torch.empty(tuple(expert_ids.shape) + (W_q.shape[2] // 2,), device=x.device, dtype=x.dtype)


@torch.library.custom_op("gemlite::experts_combine", mutates_args=())
def experts_combine(y: Tensor, expert_ids: Tensor, weights: Tensor, n_experts: int) -> Tensor:
    return _combine_impl(y, expert_ids, weights, n_experts)


@torch.library.register_fake("gemlite::experts_combine")
def _experts_combine_fake(y, expert_ids, weights, n_experts):
    _combine_check(y, expert_ids, weights)
    return torch.empty(tuple(expert_ids.shape[:-1]) + (y.shape[-1],), device=y.device, dtype=y.dtype)


# ---- the router's top-k (gemlite_hip_experts_topk): logits -> (ids, weights) in one launch ----
TOPK_SCORING = {"softmax": _hip.EXPERTS_TOPK_SOFTMAX, "sigmoid": _hip.EXPERTS_TOPK_SIGMOID}
TOPK_DOMAIN = ("domain: fp16 / bf16 / fp32 logits [..., E] with 1 <= E <= %d, 1 <= top_k <= min(E, %d), int32 / int64 ids, "
               "fp32 / fp16 / bf16 weights, an fp32 bias [E] with sigmoid scoring only"
               % (_hip.EXPERTS_TOPK_MAX_EXPERTS, _hip.EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN))


def _topk_check(logits: Tensor, top_k: int, scoring: str, bias: Optional[Tensor], ids_dtype, weights_dtype):
    if scoring not in TOPK_SCORING:
        raise ValueError(f"scoring is {scoring!r}: 'softmax' or 'sigmoid'")
    if logits.dim() < 1:
        raise ValueError("logits should be [..., E]")
    E = logits.shape[-1]
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise NotImplementedError(f"logits are {logits.dtype}: float16, bfloat16 or float32")
    if ids_dtype not in (torch.int32, torch.int64):
        raise NotImplementedError(f"ids_dtype is {ids_dtype}: int32 or int64")
    if weights_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"weights_dtype is {weights_dtype}: float32, float16 or bfloat16")
    if not 1 <= E <= _hip.EXPERTS_TOPK_MAX_EXPERTS:
        raise NotImplementedError(f"experts_topk: {E} experts ({TOPK_DOMAIN})")
    if not 1 <= top_k <= min(E, _hip.EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN):
        raise NotImplementedError(f"experts_topk: top_k={top_k} of {E} experts ({TOPK_DOMAIN})")
    if bias is not None:
        if scoring != "sigmoid":
            raise ValueError("a selection bias goes with scoring='sigmoid' only")
        if bias.dtype != torch.float32 or tuple(bias.shape) != (E,):
            raise ValueError(f"bias is {bias.dtype} {tuple(bias.shape)}: float32 ({E},)")


def _topk_impl(logits: Tensor, top_k: int, scoring: str, renormalize: bool, scale: float, bias: Optional[Tensor], ids_dtype,
               weights_dtype):
    lib = _hip.load()
    _topk_check(logits, top_k, scoring, bias, ids_dtype, weights_dtype)
    tensors = ((logits, "logits"),) + (() if bias is None else ((bias, "bias"),))
    for t, name in tensors:
        _hip.require_gpu_tensor(t, name)
    if bias is not None and bias.device != logits.device:
        raise _hip.GemliteHipError(f"logits are on {logits.device}, bias on {bias.device}")
    lead, E = tuple(logits.shape[:-1]), logits.shape[-1]
    ids = torch.empty(lead + (top_k,), dtype=ids_dtype, device=logits.device)
    weights = torch.empty(lead + (top_k,), dtype=weights_dtype, device=logits.device)
    if ids.numel() == 0:
        return ids, weights
    l2 = _rows_of(logits)
    if l2.shape[0] > 1 and l2.stride(0) < E:  # (an expanded row: the library takes row strides >= E)
        l2 = l2.contiguous()
    t = _hip.ExpertsTopkArgs()
    t.struct_size = _hip.C.sizeof(_hip.ExpertsTopkArgs)
    t.logits_dtype = TORCH_TO_DTYPE[l2.dtype].value
    t.ids_dtype, t.weights_dtype = TORCH_TO_DTYPE[ids_dtype].value, TORCH_TO_DTYPE[weights_dtype].value
    t.scoring, t.renormalize, t.scale = TOPK_SCORING[scoring], int(bool(renormalize)), float(scale)
    t.logits, t.ids, t.weights = l2.data_ptr(), ids.data_ptr(), weights.data_ptr()
    if bias is not None:
        bias = bias.contiguous()
        t.bias = bias.data_ptr()
    t.n_tokens, t.n_experts, t.top_k = l2.shape[0], E, top_k
    t.stride_logits_token = max(l2.stride(0), E)
    with _hip.on_device(logits.device):
        rc = lib.gemlite_hip_experts_topk(_hip.C.byref(t), _hip.current_stream_handle(logits.device))
    if rc in (_hip.ERR_BAD_SHAPE, _hip.ERR_UNSUPPORTED):
        raise NotImplementedError(f"gemlite_hip_experts_topk: logits {tuple(logits.shape)}, top_k={top_k}: {_hip.status_string(rc)} ({TOPK_DOMAIN})")
    _hip.raise_for_status(rc, "gemlite_hip_experts_topk")
    return ids, weights


@torch.library.custom_op("gemlite::experts_topk", mutates_args=())
def _experts_topk_op(logits: Tensor, top_k: int, scoring: str, renormalize: bool, scale: float, bias: Optional[Tensor],
                     ids_dtype: torch.dtype, weights_dtype: torch.dtype) -> Tuple[Tensor, Tensor]:
    return _topk_impl(logits, top_k, scoring, renormalize, scale, bias, ids_dtype, weights_dtype)


@torch.library.register_fake("gemlite::experts_topk")
def _experts_topk_fake(logits, top_k, scoring, renormalize, scale, bias, ids_dtype, weights_dtype):
    _topk_check(logits, top_k, scoring, bias, ids_dtype, weights_dtype)
    shape = tuple(logits.shape[:-1]) + (top_k,)
    return torch.empty(shape, device=logits.device, dtype=ids_dtype), torch.empty(shape, device=logits.device, dtype=weights_dtype)


def experts_topk(logits: Tensor, top_k: int, scoring: str = "softmax", renormalize: bool = True, scale: float = 1.0,
                 bias: Optional[Tensor] = None, ids_dtype: torch.dtype = torch.int32, weights_dtype: torch.dtype = torch.float32):
    """Router logits ``[..., E]`` -> ``(ids, weights)``, both ``[..., top_k]``, in ONE launch (``gemlite_hip_experts_topk``, DESIGN.md
    §3.1.5): what ``GemLiteExperts`` / ``GemLiteExpertsMLP`` take as ``topk_ids`` and ``topk_weights``.  ``scoring='softmax'``: the weights
    are the softmax of the logits over the selected experts (``renormalize``) or over all; ``'sigmoid'``: ``sigmoid(logit)``, selected by
    ``sigmoid(logit) + bias`` where a ``bias`` (float32 ``[E]``) is given, divided by their sum with ``renormalize``; then times ``scale``.
    Ids are distinct, in ``[0, E)`` and in descending order of the key (ties: the lower index) for every input, NaN rows included.
    A non-unit inner stride, or leading dimensions without one row stride, are copied.  There is no CPU path."""
    top_k = int(top_k)
    if torch.compiler.is_compiling():
        ids, weights = _experts_topk_op(logits, top_k, scoring, bool(renormalize), float(scale), bias, ids_dtype, weights_dtype)
        return ids, weights
    return _topk_impl(logits, top_k, scoring, renormalize, scale, bias, ids_dtype, weights_dtype)


class ExpertsRouter(torch.nn.Module):
    """``router(logits)`` -> ``(ids, weights)``: ``experts_topk`` with its settings kept; ``bias`` (float32 ``[E]``, sigmoid scoring) is a
    buffer, so it moves and saves with the model."""

    def __init__(self, top_k: int, scoring: str = "softmax", renormalize: bool = True, scale: float = 1.0, bias: Optional[Tensor] = None,
                 weights_dtype: torch.dtype = torch.float32):
        super().__init__()
        if scoring not in TOPK_SCORING:
            raise ValueError(f"scoring is {scoring!r}: 'softmax' or 'sigmoid'")
        if not 1 <= int(top_k) <= _hip.EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN:
            raise NotImplementedError(f"ExpertsRouter: top_k={top_k} ({TOPK_DOMAIN})")
        if bias is not None:
            if scoring != "sigmoid":
                raise ValueError("a selection bias goes with scoring='sigmoid' only")
            if bias.dim() != 1:
                raise ValueError(f"bias is {tuple(bias.shape)}: one float32 entry per expert")
            bias = bias.detach().to(torch.float32).contiguous()
        self.top_k, self.scoring, self.renormalize, self.scale = int(top_k), scoring, bool(renormalize), float(scale)
        self.weights_dtype = weights_dtype
        self.register_buffer("bias", bias)

    def forward(self, logits: Tensor):
        return experts_topk(logits, self.top_k, self.scoring, self.renormalize, self.scale, self.bias, torch.int32, self.weights_dtype)

    def extra_repr(self):
        return (f"top_k={self.top_k}, scoring={self.scoring!r}, renormalize={self.renormalize}, scale={self.scale}, "
                f"bias={self.bias is not None}, weights_dtype={self.weights_dtype}")


class ExpertsRouting:
    """The work table of one set of expert ids (``GemLiteExperts.route``): the slots sorted into work blocks of at most
    ``rows_per_block`` slots of one expert, on the GPU.  Owns the workspace tensor; valid for every ``GemLiteExperts`` with ``n_experts``
    experts that takes ``rows_per_block`` — the two stacks of an MLP share one.  The table is written when the route launch RUNS: inside
    a captured graph it follows the ids of every replay."""
    __slots__ = ("workspace", "rows_per_block", "n_slots", "n_experts")

    def __init__(self, workspace: Tensor, rows_per_block: int, n_slots: int, n_experts: int):
        if rows_per_block not in ROWS_PER_BLOCK:
            raise ValueError(f"rows_per_block is {rows_per_block}: one of {ROWS_PER_BLOCK}")
        need = rows_workspace_ints(max(n_slots, 1), n_experts, rows_per_block)
        if workspace.dtype != torch.int32 or workspace.dim() != 1 or workspace.numel() < need:
            raise ValueError(f"the workspace is {workspace.dtype} {tuple(workspace.shape)}: {n_slots} slots over {n_experts} experts in "
                             f"blocks of {rows_per_block} need {need} int32 entries")
        self.workspace, self.rows_per_block, self.n_slots, self.n_experts = workspace, int(rows_per_block), int(n_slots), int(n_experts)

    @property
    def blocks_max(self) -> int:
        return rows_blocks_max(max(self.n_slots, 1), self.n_experts, self.rows_per_block)

    def __repr__(self):
        return f"ExpertsRouting(n_slots={self.n_slots}, n_experts={self.n_experts}, rows_per_block={self.rows_per_block})"


class GemLiteExperts(torch.nn.Module):
    """E stacked A16W4 layers; ``experts(x, expert_ids)`` -> ``[..., top_k, N]`` in one launch (module docstring).
    ``forward_glu`` / ``forward_combine`` are the same launch with the rest of an expert MLP in its epilogue (GemLiteExpertsMLP)."""

    def __init__(self):
        super().__init__()
        self.W_q = self.scales = self.zeros = self.bias = None
        self.metadata = self.orig_shape = self.n_experts = None
        self._meta: List[int] = []
        self._views: dict = {}
        self._fused_ok: dict = {}

    # ---------------------------------------------------------------------------------------- build
    @staticmethod
    def _check_same(layers: list) -> list:
        """-> the meta args all `layers` share; refuses layers that differ in them or in the shape, dtype or device of a tensor."""
        if not layers:
            raise ValueError("from_layers needs at least one layer")
        first = layers[0]
        if getattr(first, "elements_per_sample", None) is None or not isinstance(getattr(first, "W_q", None), Tensor):
            raise ValueError("from_layers takes packed GemLiteLinear layers (call .pack() first)")
        meta = first.get_meta_args()

        def same(a: Optional[Tensor], b: Optional[Tensor]) -> bool:
            if a is None or b is None:
                return a is b
            return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device

        for i, layer in enumerate(layers[1:], 1):
            if getattr(layer, "elements_per_sample", None) is None or layer.get_meta_args() != meta:
                raise ValueError(f"layer {i} differs from layer 0 in bits, group size, modes or dtypes: "
                                 f"{getattr(layer, 'elements_per_sample', None) and layer.get_meta_args()} vs {meta}")
            for name in ("W_q", "scales", "zeros", "bias"):
                if not same(getattr(layer, name), getattr(first, name)):
                    raise ValueError(f"layer {i} differs from layer 0 in the shape, dtype or device of `{name}`")
        if first.zeros.numel() == 1 and any(int(l.zeros) != int(first.zeros) for l in layers[1:]):
            raise ValueError("the layers carry different scalar zeros: one scalar zero is shared by all experts")
        return meta

    @classmethod
    def from_layers(cls, layers: Sequence["core.GemLiteLinearHIP"], del_orig: bool = False) -> "GemLiteExperts":
        layers = list(layers)
        meta = cls._check_same(layers)
        first = layers[0]
        stack = lambda name: torch.stack([getattr(l, name).data for l in layers]).contiguous()  # noqa: E731
        W_q = stack("W_q")
        scales = stack("scales") if first.scales.numel() > 0 else first.scales.data
        zeros = stack("zeros") if first.zeros.numel() > 1 else first.zeros.data
        bias = None if first.bias is None else stack("bias")
        self = cls._from_stacked(meta, W_q, scales, zeros, bias, first.out_features, first.in_features)
        if del_orig:
            for layer in layers:
                layer.W_q = layer.scales = layer.zeros = layer.bias = None
        return self

    @classmethod
    def from_gate_up(cls, gate_layers: Sequence["core.GemLiteLinearHIP"], up_layers: Sequence["core.GemLiteLinearHIP"],
                     del_orig: bool = False) -> "GemLiteExperts":
        """Experts whose layer e is gate e and up e side by side along N — columns [0, I) the gate, [I, 2 I) the up, the w13 layout
        ``forward_glu`` reads.  The packing runs along K, so the packed words, scales, zeros and bias concatenate on their last axis."""
        gate_layers, up_layers = list(gate_layers), list(up_layers)
        if len(gate_layers) != len(up_layers):
            raise ValueError(f"{len(gate_layers)} gate layers, {len(up_layers)} up layers")
        meta = cls._check_same(gate_layers + up_layers)
        first = gate_layers[0]
        pair = lambda name: torch.stack([torch.cat([getattr(g, name).data, getattr(u, name).data], dim=-1)  # noqa: E731
                                         for g, u in zip(gate_layers, up_layers)]).contiguous()
        W_q = pair("W_q")
        scales = pair("scales") if first.scales.numel() > 0 else first.scales.data
        zeros = pair("zeros") if first.zeros.numel() > 1 else first.zeros.data
        bias = None if first.bias is None else pair("bias")
        self = cls._from_stacked(meta, W_q, scales, zeros, bias, 2 * first.out_features, first.in_features)
        if del_orig:
            for layer in gate_layers + up_layers:
                layer.W_q = layer.scales = layer.zeros = layer.bias = None
        return self

    @classmethod
    def _from_stacked(cls, meta, W_q: Tensor, scales: Tensor, zeros: Tensor, bias: Optional[Tensor], out_features: int,
                      in_features: int) -> "GemLiteExperts":
        self = cls()
        self._meta = [int(v) for v in meta]
        self._check_domain(W_q, scales, zeros, bias)
        as_param = lambda t: torch.nn.Parameter(t, requires_grad=False)  # noqa: E731
        dev = W_q.device
        self.W_q = as_param(W_q)
        self.bias = None if bias is None else as_param(bias)
        self.scales, self.zeros = as_param(scales), as_param(zeros)
        self.metadata = as_param(torch.tensor(self._meta, device=dev, dtype=torch.int32))
        self.orig_shape = as_param(torch.tensor([out_features, in_features], device=dev, dtype=torch.int32))
        self.n_experts = as_param(torch.tensor(W_q.shape[0], device=dev, dtype=torch.int32))
        self._set_shapes(out_features, in_features, W_q.shape[0])
        return self

    def _set_shapes(self, out_features: int, in_features: int, n: int):
        self.out_features, self.in_features, self.num_experts = int(out_features), int(in_features), int(n)
        self._views = {}
        self._fused_ok = {}

    def _check_domain(self, W_q: Tensor, scales: Tensor, zeros: Tensor, bias: Optional[Tensor]):
        """The library's own answer (gemlite_hip_experts_query plans and never launches, with or without a GPU), on the stacked tensors
        with stand-ins for x / out / ids; the most common refusals first, in words."""
        m = self._meta
        if m[0] or m[5] not in (DType.FP16.value, DType.BF16.value) or m[6] != m[5]:
            raise NotImplementedError("GemLiteExperts: weight-only layers with fp16 / bf16 activations and outputs of the same type")
        if m[1] != 4 or m[4] != 8 or W_q.dtype != torch.int32:
            raise NotImplementedError(f"GemLiteExperts: 4-bit weights packed in 32-bit words (W_nbits={m[1]}, {W_q.dtype} words)")
        if m[9] != 0 or not 1 <= m[10] <= 4:
            raise NotImplementedError(f"GemLiteExperts: grouped scales / zeros (W_group_mode 1..4, no channel scales); "
                                      f"got W_group_mode={m[10]}, channel_scale_mode={m[9]}")
        e = _static_args(W_q, scales, zeros, bias, m)
        e.layer.x = e.layer.out = e.ids = 0x1000
        e.layer.stride_xm = e.stride_x_row = e.layer.K
        e.ids_dtype = DType.INT32.value
        e.n_slots = e.slots_per_x_row = 1
        e.stride_out_slot = e.layer.N
        rc = _hip.load().gemlite_hip_experts_query(_hip.C.byref(e))
        if rc != _hip.OK:
            raise NotImplementedError(f"GemLiteExperts: N={e.layer.N} K={e.layer.K} group_size={m[2]} W_group_mode={m[10]}: "
                                      f"{_hip.status_string(rc)} (domain: N % 16 == 0, K % 256 == 0, a power-of-two group_size >= 32, "
                                      "16-byte aligned contiguous weights)")

    # ------------------------------------------------------------------------------- (de)serialise
    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.W_q = state_dict.pop("W_q", None)
        self.bias = state_dict.pop("bias", None)
        self.scales = state_dict.pop("scales", None)
        self.zeros = state_dict.pop("zeros", None)
        self.metadata = state_dict.pop("metadata")
        self.orig_shape = state_dict.pop("orig_shape")
        self.n_experts = state_dict.pop("n_experts")
        self._meta = [int(v) for v in self.metadata]
        out_features, in_features = (int(v) for v in self.orig_shape)
        if int(self.n_experts) != self.W_q.shape[0]:
            raise ValueError(f"n_experts is {int(self.n_experts)}, W_q holds {self.W_q.shape[0]} experts")
        self._set_shapes(out_features, in_features, self.W_q.shape[0])
        self._check_domain(self.W_q, self.scales, self.zeros, self.bias)

    # ----------------------------------------------------------------------------------- arguments
    def get_tensor_args(self):
        return [self.W_q, self.scales, self.zeros]

    def get_meta_args(self):
        return list(self._meta)

    def expert(self, e: int) -> "core.GemLiteLinearHIP":
        """A GemLiteLinear VIEW on expert e's slices (no copy): per-expert calls, tests, dequantize()."""
        e = int(e)
        if not 0 <= e < self.num_experts:
            raise IndexError(f"expert {e} of {self.num_experts}")
        lin = self._views.get(e)
        if lin is None:
            m = self._meta
            lin = core.GemLiteLinearHIP(m[1], m[2], self.in_features, self.out_features, DType(m[5]), DType(m[6]))
            lin.load_state_dict({
                "W_q": self.W_q.data[e], "bias": None if self.bias is None else self.bias.data[e],
                "scales": self.scales.data[e] if self.scales.dim() == 3 else self.scales.data,
                "zeros": self.zeros.data[e] if self.zeros.dim() == 3 else self.zeros.data,
                "metadata": list(m), "orig_shape": (self.out_features, self.in_features)})
            self._views[e] = lin
        return lin

    # ------------------------------------------------------------------------------------- forward
    def forward(self, x: Tensor, expert_ids: Tensor) -> Tensor:
        if x.dtype != DTYPE_TO_TORCH[self._meta[5]]:
            raise NotImplementedError(f"GemLiteExperts: x is {x.dtype}, the experts take {DTYPE_TO_TORCH[self._meta[5]]}")
        if torch.compiler.is_compiling():
            return forward_experts(x, expert_ids, self.bias, self.get_tensor_args(), self._meta)
        return _forward_impl(x, expert_ids, self.bias, self.get_tensor_args(), self._meta)

    # ------------------------------------------------------------------------------------- batches
    def rows_per_block(self, n_slots: int, rows_per_block: Optional[int] = None, glu: bool = False) -> int:
        """The work-block size R the library resolves for `n_slots` slots on these experts (None: its default); host only.
        ``glu=True``: the answer for ``forward_batched_glu``, whose two-tile blocks cap groups of 64 at 32 rows and have no form for
        groups of 32 (NotImplementedError)."""
        if glu:
            return _resolve_rows_glu(self.bias, self.get_tensor_args(), self._meta, n_slots, rows_per_block)
        return _resolve_rows(self.bias, self.get_tensor_args(), self._meta, n_slots, rows_per_block)

    def route(self, expert_ids: Tensor, rows_per_block: Optional[int] = None) -> ExpertsRouting:
        """Sort the slots of ``expert_ids`` by expert into work blocks, in ONE launch that reads the ids on the GPU (no host
        synchronisation; capturable).  The result feeds ``forward_batched`` of every stack with as many experts that takes its R."""
        if expert_ids.dim() < 1:
            raise ValueError("expert_ids should be [..., top_k]")
        n_slots = expert_ids.numel()
        if n_slots > MAX_SLOTS:
            raise NotImplementedError(f"GemLiteExperts.route: {n_slots} slots; one routing holds at most {MAX_SLOTS}")
        R = self.rows_per_block(n_slots, rows_per_block)
        if torch.compiler.is_compiling():
            ws = experts_route(expert_ids, R, self.bias, self.get_tensor_args(), self._meta)
        else:
            ws = _route_impl(expert_ids, R, self.bias, self.get_tensor_args(), self._meta)
        return ExpertsRouting(ws, R, n_slots, self.num_experts)

    def forward_batched(self, x: Tensor, expert_ids: Tensor, routing: Optional[ExpertsRouting] = None) -> Tensor:
        """-> ``[..., top_k, N]`` like ``forward``, for MORE THAN ONE token: every expert's weights stream once per work block of the
        routing through the MFMA rows kernel.  A valid slot is bit-identical to its row of that expert's own rows-kernel launch (NOT to
        ``forward``, whose decode kernel sums K in another order); a slot with an id outside [0, E) is a row of zeros."""
        self._check_x(x)
        if expert_ids.dim() < 1:
            raise ValueError("expert_ids should be [..., top_k]")
        _split(x, expert_ids, self.in_features)
        if routing is None:
            routing = self.route(expert_ids)
        elif not isinstance(routing, ExpertsRouting):
            raise TypeError(f"routing is a {type(routing).__name__}: an ExpertsRouting from GemLiteExperts.route, or None")
        if routing.n_slots != expert_ids.numel() or routing.n_experts != self.num_experts:
            raise ValueError(f"the routing holds {routing.n_slots} slots over {routing.n_experts} experts; expert_ids has "
                             f"{expert_ids.numel()} slots and these are {self.num_experts} experts")
        if routing.rows_per_block > 32 and self._meta[2] == 32:
            raise NotImplementedError(f"the routing has work blocks of {routing.rows_per_block} rows: groups of 32 take 16 or 32 "
                                      "(route with rows_per_block=32, or with the stack of the smaller group size)")
        args = (x, expert_ids, routing.workspace, routing.rows_per_block, self.bias, self.get_tensor_args(), self._meta)
        return forward_experts_rows(*args) if torch.compiler.is_compiling() else _forward_rows_impl(*args)

    def forward_batched_glu(self, x: Tensor, expert_ids: Tensor, routing: Optional[ExpertsRouting] = None) -> Tensor:
        """-> ``[..., top_k, N // 2]``: ``silu(y[..., :I]) * y[..., I:]`` of ``y = forward_batched(x, expert_ids, routing)`` — fp32 on the
        rounded values, one rounding — in the same one launch; no ``[..., top_k, N]`` intermediate exists.  Experts stacked
        ``[gate; up]`` along N (``from_gate_up``).  Out of the domain (N % 32, groups of 32, a routing above the GLU cap): NotImplementedError."""
        self._check_x(x)
        if expert_ids.dim() < 1:
            raise ValueError("expert_ids should be [..., top_k]")
        _split(x, expert_ids, self.in_features)
        if routing is None:
            n_slots = expert_ids.numel()
            if n_slots > MAX_SLOTS:
                raise NotImplementedError(f"GemLiteExperts.forward_batched_glu: {n_slots} slots; one routing holds at most {MAX_SLOTS}")
            routing = self.route(expert_ids, self.rows_per_block(n_slots, glu=True))
        elif not isinstance(routing, ExpertsRouting):
            raise TypeError(f"routing is a {type(routing).__name__}: an ExpertsRouting from GemLiteExperts.route, or None")
        if routing.n_slots != expert_ids.numel() or routing.n_experts != self.num_experts:
            raise ValueError(f"the routing holds {routing.n_slots} slots over {routing.n_experts} experts; expert_ids has "
                             f"{expert_ids.numel()} slots and these are {self.num_experts} experts")
        self.rows_per_block(max(routing.n_slots, 1), routing.rows_per_block, glu=True)  # the library's refusals, in words (host only)
        args = (x, expert_ids, routing.workspace, routing.rows_per_block, self.bias, self.get_tensor_args(), self._meta)
        return forward_experts_rows_glu(*args) if torch.compiler.is_compiling() else _forward_rows_glu_impl(*args)

    def combine_batched(self, y: Tensor, expert_ids: Tensor, weights: Tensor) -> Tensor:
        """-> ``[..., N]``: ``sum_k weights[..., k] * y[..., k, :]`` over the slots with an id in [0, E), in ONE launch — fp32 products and
        adds in ascending k, one rounding: on the same ``y`` the bits of ``forward_combine``.  ``y`` is any ``[..., top_k, N]`` output of
        ``forward_batched`` or ``forward`` (views with a unit inner stride are read in place); invalid slots are skipped unread."""
        if torch.compiler.is_compiling():
            return experts_combine(y, expert_ids, weights, self.num_experts)
        return _combine_impl(y, expert_ids, weights, self.num_experts)

    def _check_fused(self, epilogue: int, top_k: int):
        """The library's answer for a fused epilogue on these experts (gemlite_hip_experts_fused_query on stand-ins, as _check_domain asks
        it), once per (epilogue, top_k), in words."""
        rc = self._fused_ok.get((epilogue, top_k))
        if rc is None:
            e = _static_args(self.W_q, self.scales, self.zeros, self.bias, self._meta)
            e.layer.x = e.layer.out = e.ids = 0x1000
            e.layer.stride_xm = e.stride_x_row = e.layer.K
            e.ids_dtype = DType.INT32.value
            e.n_slots, e.slots_per_x_row = max(top_k, 1), 1
            e.stride_out_slot = e.layer.N
            f = _fused_args(e, epilogue, 0x1000, DType.FP32.value, top_k)
            rc = self._fused_ok[(epilogue, top_k)] = _hip.load().gemlite_hip_experts_fused_query(_hip.C.byref(f))
        if rc != _hip.OK:
            what = (f"forward_glu: N={self.out_features} (domain: N % 32 == 0, the [gate; up] halves in whole 16-column tiles)"
                    if epilogue == _hip.EXPERTS_GLU else f"forward_combine: top_k={top_k} (domain: 1 <= top_k <= 16; top_k > 16 is not fused)")
            raise NotImplementedError(f"GemLiteExperts.{what}: {_hip.status_string(rc)}")

    def _check_x(self, x: Tensor):
        if x.dtype != DTYPE_TO_TORCH[self._meta[5]]:
            raise NotImplementedError(f"GemLiteExperts: x is {x.dtype}, the experts take {DTYPE_TO_TORCH[self._meta[5]]}")

    def forward_glu(self, x: Tensor, expert_ids: Tensor) -> Tensor:
        """-> ``[..., top_k, N // 2]``: ``silu(y[..., :I]) * y[..., I:]`` of ``y = forward(x, expert_ids)``, in the same one launch."""
        self._check_x(x)
        if torch.compiler.is_compiling():
            return forward_experts_glu(x, expert_ids, self.bias, self.get_tensor_args(), self._meta)
        self._check_fused(_hip.EXPERTS_GLU, 1)
        return _fused_impl(_hip.EXPERTS_GLU, x, expert_ids, None, self.bias, self.get_tensor_args(), self._meta)

    def forward_combine(self, x: Tensor, expert_ids: Tensor, weights: Tensor) -> Tensor:
        """-> ``[..., N]``: ``(forward(x, expert_ids) * weights.unsqueeze(-1)).sum(-2)`` with an fp32 sum, in the same one launch."""
        self._check_x(x)
        if expert_ids.dim() < 1:
            raise ValueError("expert_ids should be [..., top_k]")
        if torch.compiler.is_compiling():
            return forward_experts_combine(x, expert_ids, weights, self.bias, self.get_tensor_args(), self._meta)
        self._check_fused(_hip.EXPERTS_COMBINE, max(int(expert_ids.shape[-1]), 1))
        return _fused_impl(_hip.EXPERTS_COMBINE, x, expert_ids, weights, self.bias, self.get_tensor_args(), self._meta)


class GemLiteExpertsMLP(torch.nn.Module):
    """The expert MLP of a mixture-of-experts layer in two launches: ``mlp(x, topk_ids, topk_weights)`` -> ``[..., hidden]`` is
    ``down.forward_combine(gate_up.forward_glu(x, ids), ids, w)``.  ``gate_up`` holds [gate; up] along N (GemLiteExperts.from_gate_up).
    Without arguments: an empty module for ``load_state_dict``."""

    def __init__(self, gate_up: Optional[GemLiteExperts] = None, down: Optional[GemLiteExperts] = None):
        super().__init__()
        if (gate_up is None) != (down is None):
            raise ValueError("GemLiteExpertsMLP takes both gate_up and down, or neither (load_state_dict fills them)")
        self.gate_up = GemLiteExperts() if gate_up is None else gate_up
        self.down = GemLiteExperts() if down is None else down
        if gate_up is not None:
            self._check()

    def _check(self):
        g, d = self.gate_up, self.down
        if g.out_features != 2 * d.in_features:
            raise ValueError(f"gate_up has {g.out_features} outputs, down {d.in_features} inputs: gate_up.out_features == 2 * down.in_features")
        if d.out_features != g.in_features:
            raise ValueError(f"down has {d.out_features} outputs, gate_up {g.in_features} inputs: the MLP maps hidden to hidden")
        if g.num_experts != d.num_experts:
            raise ValueError(f"gate_up holds {g.num_experts} experts, down {d.num_experts}")
        if g.get_meta_args()[5] != d.get_meta_args()[5] or g.W_q.device != d.W_q.device:
            raise ValueError("gate_up and down differ in dtype or device")
        self.hidden_size, self.intermediate_size, self.num_experts = g.in_features, d.in_features, g.num_experts

    @classmethod
    def from_layers(cls, gate_layers, up_layers, down_layers, del_orig: bool = False) -> "GemLiteExpertsMLP":
        return cls(GemLiteExperts.from_gate_up(gate_layers, up_layers, del_orig), GemLiteExperts.from_layers(down_layers, del_orig))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        for name in ("gate_up", "down"):
            prefix = name + "."
            getattr(self, name).load_state_dict({k[len(prefix):]: state_dict.pop(k) for k in list(state_dict) if k.startswith(prefix)})
        self._check()

    def forward(self, x: Tensor, topk_ids: Tensor, topk_weights: Tensor) -> Tensor:
        return self.down.forward_combine(self.gate_up.forward_glu(x, topk_ids), topk_ids, topk_weights)

    def forward_routed(self, x: Tensor, logits: Tensor, router: "ExpertsRouter") -> Tensor:
        """``self(x, *router(logits))``: router logits to ``[..., hidden]`` in three launches, no torch arithmetic between them."""
        return self(x, *router(logits))

    def forward_batched_fused_routed(self, x: Tensor, logits: Tensor, router: "ExpertsRouter") -> Tensor:
        """``self.forward_batched_fused(x, *router(logits))``: five launches for a batch of tokens."""
        return self.forward_batched_fused(x, *router(logits))

    def rows_per_block(self, n_slots: int) -> int:
        """The work-block size both stacks take: each one's own default where they agree, else the smaller (valid for both: only the
        cap of groups of 32 separates the defaults of two stacks with the same experts and slots)."""
        return min(self.gate_up.rows_per_block(n_slots), self.down.rows_per_block(n_slots))

    def glu_fused(self) -> bool:
        """Whether ``gate_up`` has a GLU form of the batched launch (N % 32 == 0 and groups of 64 or more); host only."""
        try:
            self.gate_up.rows_per_block(1, glu=True)
        except NotImplementedError:
            return False
        return True

    def rows_per_block_fused(self, n_slots: int) -> int:
        """The work-block size ``forward_batched_fused`` routes with (host only): the smaller of gate_up's GLU answer and down's plain
        answer — valid for both, since a stack takes every R up to its cap.  Where gate_up has no GLU form: ``rows_per_block``."""
        if not self.glu_fused():
            return self.rows_per_block(n_slots)
        return min(self.gate_up.rows_per_block(n_slots, glu=True), self.down.rows_per_block(n_slots))

    def forward_batched_fused(self, x: Tensor, topk_ids: Tensor, topk_weights: Tensor) -> Tensor:
        """``forward_batched`` in four launches and without an fp32 intermediate in memory: ONE route, ``gate_up.forward_batched_glu``
        (SwiGLU inside the rows launch), ``down.forward_batched`` on the SAME routing, ``down.combine_batched`` -> ``[..., hidden]``.
        Where gate_up is outside the GLU domain (groups of 32) the gate/up launch and the torch SwiGLU of ``forward_batched`` stand in
        for the second launch; the combine is one launch all the same."""
        if topk_ids.dim() < 1:
            raise ValueError("topk_ids should be [..., top_k]")
        _weights_like(topk_weights, topk_ids, x)
        routing = self.gate_up.route(topk_ids, self.rows_per_block_fused(topk_ids.numel()))
        if self.glu_fused():
            h = self.gate_up.forward_batched_glu(x, topk_ids, routing)
        else:
            y = self.gate_up.forward_batched(x, topk_ids, routing).float()
            inter = self.intermediate_size
            h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(x.dtype)
        return self.down.combine_batched(self.down.forward_batched(h, topk_ids, routing), topk_ids, topk_weights)

    def forward_batched(self, x: Tensor, topk_ids: Tensor, topk_weights: Tensor) -> Tensor:
        """``forward`` for MORE THAN ONE token: ONE route, ``gate_up.forward_batched``, ``silu(gate) * up`` in torch (fp32, one rounding),
        ``down.forward_batched`` on the SAME routing, the routing-weight sum in torch (fp32, one rounding) -> ``[..., hidden]``."""
        if topk_ids.dim() < 1:
            raise ValueError("topk_ids should be [..., top_k]")
        _weights_like(topk_weights, topk_ids, x)
        routing = self.gate_up.route(topk_ids, self.rows_per_block(topk_ids.numel()))
        y = self.gate_up.forward_batched(x, topk_ids, routing).float()
        inter = self.intermediate_size
        h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(x.dtype)
        d = self.down.forward_batched(h, topk_ids, routing).float()
        return (d * topk_weights.float().unsqueeze(-1)).sum(-2).to(x.dtype)
