"""Tensor-level wrappers over the C ABI (``include/bgs.h``).

PyTorch is plumbing here: device memory, the current HIP stream and autograd graph
edges.  All arithmetic happens in the hand-written gfx950 kernels of ``libbgs.so``.
Every wrapper requires CUDA(ROCm) tensors and raises otherwise — there is no CPU
path in the product.
"""
import ctypes
import itertools
import math
import os

import torch

from . import capi

_WS = {}


def _workspace(nbytes, device):
    """Per (device, stream) scratch buffer; kernels of one stream are serialised."""
    key = (device.index, capi.raw_stream(device))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def reset_workspaces():
    """Drop every cached scratch buffer.  Call before capturing a NEW hipGraph in a process that
    already captured one: a buffer handed out during an earlier capture lives in that graph's
    private memory pool and must not be baked into another graph."""
    _WS.clear()


_SIDE = {}
_PIPELINE_ACTIVE = [0]      # non-zero (the id of the owning train.TrunkPipeline) while one has batches in flight


def level_fork_enabled():
    """Small pyramid levels on a side stream (FPN output convs, RPN head): ``BGS_LEVEL_FORK=0`` turns it off.  Off as
    well while a ``train.TrunkPipeline`` has batches in flight: its pieces already run on three or four streams, and
    forks inside every one of them oversubscribe the hardware queues (depth 3: 6.17 ms per step with the inner
    forks, 5.74 without; profiles/r9h)."""
    return os.environ.get('BGS_LEVEL_FORK', '1') != '0' and not _PIPELINE_ACTIVE[0]


def shortcut_fork_enabled():
    """Projection shortcuts of frozen residual blocks on the side stream (backbone.Bottleneck.run):
    ``BGS_SHORTCUT_FORK=0`` turns it off (``BGS_LEVEL_FORK=0`` turns every fork off)."""
    return level_fork_enabled() and os.environ.get('BGS_SHORTCUT_FORK', '1') != '0'


def rpn_loss_fork_enabled():
    """The RPN loss chain (~12 short dependent launches) on the side stream (detectors._rpn_forward_train).  Default
    ``BGS_RPN_LOSS_FORK=auto``: when launching eagerly (two real streams: 6.45 -> 6.30 ms per step), not while a
    hipGraph is being captured (inside a replayed graph the fork's event edges cost more than the overlap returns:
    6.44 -> 6.49 ms); ``1`` / ``0`` force it."""
    v = os.environ.get('BGS_RPN_LOSS_FORK', 'auto')
    if v == 'auto':
        return level_fork_enabled() and not torch.cuda.is_current_stream_capturing()
    return level_fork_enabled() and v != '0'


class forked(object):
    """``with forked(device) as f: <launches>`` issues the block on the device's side stream, ordered after
    everything enqueued on the current stream so far; ``f.join()`` makes the current stream wait for it.

    Why: the stride-16 / 32 / 64 pyramid levels launch 168 / 48 / 16 workgroups on 256 CUs; next to the P2-level
    launch of the same layer (2100 workgroups) they fill CUs that would idle in its tail instead of taking their
    own serial slot (tools/stream_overlap_ab.py: 1.10 -> 1.02 ms for the five FPN output convs, eagerly and in
    a replayed hipGraph).  Dependent chains of tiny kernels do NOT gain from a fork (an event edge costs more than
    a back-to-back launch: 69 -> 139 us for two chains of 20), so only conv launches are forked.
    Tensors allocated inside the block belong to the side stream's pool; they are consumed after ``join()`` and
    freed after it, and the next block starts with an event recorded after those consumers: no reuse race.
    Tensors allocated on the MAIN stream that the block only reads are a different matter: if the host drops its
    last reference before ``join()``, the caching allocator may hand the block to a later main-stream allocation
    that is not ordered against the side stream.  ``hold(*tensors)`` keeps such inputs alive until ``join()``
    (which orders the main stream after the block) — every long-lived fork must hold what it reads."""

    def __init__(self, device, lane=0):
        # lane 0: short forks that are joined before the next one opens; lanes 1, 2: long-lived branches (the RPN loss
        # chain, the mask branch) that stay open across other forks — each lane is its own stream, so a short fork
        # never queues behind a long one
        # (one set of lanes PER PARENT stream: the trunk stage of train.TrunkPipeline forks its small pyramid levels from
        #  its own stream while the head stage forks from the main one — sharing a lane would queue the two stages'
        #  unrelated forks behind each other)
        key = (device.index if device.index is not None else torch.cuda.current_device(), int(lane),
               torch.cuda.current_stream(device).cuda_stream)
        if key not in _SIDE:
            _SIDE[key] = torch.cuda.Stream(device=device)
        self.side = _SIDE[key]
        self.device = device
        self.done = None
        self._held = None

    def hold(self, *tensors):
        """Keep main-stream tensors (or nests of them) that the forked block reads alive until ``join()``."""
        if self._held is None:
            self._held = []
        self._held.extend(tensors)
        return self

    def __enter__(self):
        main = torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(main)
        self.side.wait_event(ev)
        self._ctx = torch.cuda.stream(self.side)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.done = torch.cuda.Event()
        self.done.record(self.side)
        self._ctx.__exit__(*exc)
        return False

    def join(self):
        torch.cuda.current_stream(self.device).wait_event(self.done)
        # from here on every main-stream launch is ordered after the block: its inputs may be recycled
        self._held = None


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                'balancedgroupsoftmax_amd ops run only on the GPU (hand-written HIP kernels); '
                'got a %s tensor. There is no CPU fallback.' % t.device)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


# ----------------------------------------------------------------------------------------
# label remap + sampling  (GSBBoxHeadWith0._remap_labels, gs_bbox_head_with0.py:91-112)
# ----------------------------------------------------------------------------------------
_seed_counter = itertools.count(1)


def gs_prepare(labels, label2binlabel, others_sample_ratio, seed=None, cls_weight=None,
               seed_offset=None, row_weights=None):
    """Device-side ``_remap_labels``: returns ``bin_labels [B,N] i32`` (the
    ``label2binlabel[b][labels]`` gather), ``weights [B,N] f32``, ``avg [B] f32``.  No host sync.

    ``seed``: draw identifier of the counter-based RNG; ``None`` takes the next value of
    a process-wide counter mixed with ``torch.initial_seed()`` (reproducible runs).
    ``seed_offset``: optional device int64 ``[1]`` draw counter added to the seed on the
    device (bump it with a tensor op; needed under hipGraph replay where ``seed`` is frozen).
    ``row_weights``: the detector's ``label_weights [N]``; rows <= 0 are padding slots of a
    fixed-shape batch and are left out of every count, draw and loss.
    """
    _require_cuda(labels, label2binlabel, cls_weight, row_weights)
    lib = capi.load()
    labels = labels.contiguous()
    assert labels.dtype == torch.int64 and label2binlabel.dtype == torch.int64
    B, C = label2binlabel.shape
    N = labels.numel()
    dev = labels.device
    if seed is None:
        seed = (torch.initial_seed() * 0x9E3779B1 + next(_seed_counter)) & 0xFFFFFFFFFFFFFFFF
    weights = torch.empty((B, N), dtype=torch.float32, device=dev)
    avg = torch.empty((B,), dtype=torch.float32, device=dev)
    bl = torch.empty((B, N), dtype=torch.int32, device=dev)
    cw_stride = 0
    if cls_weight is not None:
        assert cls_weight.dtype == torch.float32 and cls_weight.dim() == 2
        assert cls_weight.shape[0] == B - 1 and cls_weight.is_contiguous()
        cw_stride = cls_weight.shape[1]
    if row_weights is not None:
        row_weights = _f32c(row_weights)
        assert row_weights.numel() == N
    rc = lib.bgs_gs_prepare(capi.ptr(labels), capi.ptr(label2binlabel), capi.ptr(cls_weight),
                            cw_stride, capi.ptr(row_weights), N, C, B, float(others_sample_ratio),
                            int(seed),
                            capi.ptr(seed_offset), capi.ptr(bl), capi.ptr(weights), capi.ptr(avg),
                            capi.current_stream(dev))
    capi.check('bgs_gs_prepare', rc)
    return bl, weights, avg


# ----------------------------------------------------------------------------------------
# fused group-softmax loss  (GSBBoxHeadWith0.loss classification part, :160-171)
# ----------------------------------------------------------------------------------------
def _gs_loss_launch(logits, bin_labels, pred_slice_host, weights, avg, want_grad):
    lib = capi.load()
    N, W = logits.shape
    B = bin_labels.shape[0]
    dev = logits.device
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits) if want_grad else None
    ws = _workspace(lib.bgs_gs_loss_workspace_bytes(N, B), dev)
    ps_keep, ps_ptr = capi.host_i64(pred_slice_host)
    rc = lib.bgs_gs_loss_fwd_bwd(capi.ptr(logits), capi.ptr(bin_labels), ps_ptr,
                                 capi.ptr(weights), capi.ptr(avg), N, B, W, capi.ptr(loss),
                                 capi.ptr(dlogits), capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_gs_loss_fwd_bwd', rc)
    return loss, dlogits


class _GroupSoftmaxLoss(torch.autograd.Function):
    """losses[B] = fused kernel; the gradient w.r.t. the logits is produced by the SAME
    launch and only rescaled by the upstream scalars in backward (early-out when they are 1)."""

    @staticmethod
    def forward(ctx, logits, bin_labels, pred_slice_host, weights, avg):
        want_grad = logits.requires_grad
        z = _f32c(logits)
        loss, dlogits = _gs_loss_launch(z, bin_labels, pred_slice_host, weights, avg, want_grad)
        ctx.dlogits = dlogits
        ctx.pred_slice_host = pred_slice_host
        ctx.in_dtype = logits.dtype
        ctx.prev_g = None
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        dl = ctx.dlogits
        if dl is None:
            return None, None, None, None, None
        if ctx.prev_g is not None:
            # The kernel's dlogits buffer is scaled IN PLACE and handed to autograd (no second
            # [N, W] tensor per step); a second backward through a retained graph would rescale a
            # tensor the first one already gave away (and could not recover bins whose first
            # upstream grad was 0).  Refuse instead of returning wrong gradients.
            raise RuntimeError('group_softmax_loss: the fused dlogits buffer was consumed by the '
                               'first backward; a second backward through a retained graph is not '
                               'supported — call the loss again')
        lib = capi.load()
        g = grad_loss.detach().to(torch.float32).contiguous()
        N, W = dl.shape
        ps_keep, ps_ptr = capi.host_i64(ctx.pred_slice_host)
        rc = lib.bgs_gs_scale_grad(capi.ptr(dl), ps_ptr, capi.ptr(g), N, ps_keep.shape[0], W,
                                   capi.current_stream(dl.device))
        capi.check('bgs_gs_scale_grad', rc)
        ctx.prev_g = g
        out = dl if ctx.in_dtype == torch.float32 else dl.to(ctx.in_dtype)
        return out, None, None, None, None


class _GsHeadFusedLoss(torch.autograd.Function):
    """``_remap_labels`` + ``_sample_others`` + loss + gradient in one streaming launch
    (``bgs_gs_head_loss_fused``); backward as :class:`_GroupSoftmaxLoss`."""

    @staticmethod
    def forward(ctx, logits, labels, l2b, pred_slice_host, ratio, seed, seed_offset, row_weights,
                debug):
        lib = capi.load()
        z = _f32c(logits)
        N, W = z.shape
        B, C = l2b.shape
        dev = z.device
        want_grad = logits.requires_grad
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        avg = torch.empty((B,), dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(z) if want_grad else None
        bl = torch.empty((B, N), dtype=torch.int32, device=dev) if debug else None
        w = torch.empty((B, N), dtype=torch.float32, device=dev) if debug else None
        ws = _workspace(lib.bgs_gs_loss_workspace_bytes(N, B), dev)
        ps_keep, ps_ptr = capi.host_i64(pred_slice_host)
        rw = None if row_weights is None else _f32c(row_weights)
        rc = lib.bgs_gs_head_loss_fused(capi.ptr(z), capi.ptr(labels), capi.ptr(l2b), capi.ptr(rw),
                                        ps_ptr, N, C, B, W, float(ratio), int(seed),
                                        capi.ptr(seed_offset), capi.ptr(loss), capi.ptr(dlogits),
                                        capi.ptr(avg), capi.ptr(bl), capi.ptr(w), capi.ptr(ws),
                                        capi.current_stream(dev))
        capi.check('bgs_gs_head_loss_fused', rc)
        ctx.dlogits = dlogits
        ctx.pred_slice_host = pred_slice_host
        ctx.in_dtype = logits.dtype
        ctx.prev_g = None
        ctx.mark_non_differentiable(avg)
        if debug:
            ctx.mark_non_differentiable(bl, w)
            return loss, avg, bl, w
        return loss, avg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, *_unused):
        out = _GroupSoftmaxLoss.backward(ctx, grad_loss)[0]
        return (out,) + (None,) * 8


_CLASS_BITS = {}


def gs_class_bin_mask(label2binlabel):
    """``[C]`` uint16 device table, bit b = class is foreground in bin b
    (``bgs_gs_class_bin_mask``); cached per table tensor (the tables are constants of a head)."""
    _require_cuda(label2binlabel)
    key = (label2binlabel.data_ptr(), label2binlabel._version, tuple(label2binlabel.shape))
    hit = _CLASS_BITS.get(key)
    if hit is not None:
        return hit[1]
    lib = capi.load()
    B, C = label2binlabel.shape
    out = torch.empty(((C + 7) // 8 * 8,), dtype=torch.int16, device=label2binlabel.device)   # padded: read in 16-byte pieces
    rc = lib.bgs_gs_class_bin_mask(capi.ptr(label2binlabel), C, B, capi.ptr(out),
                                   capi.current_stream(label2binlabel.device))
    capi.check('bgs_gs_class_bin_mask', rc)
    if len(_CLASS_BITS) > 64:
        _CLASS_BITS.clear()
    _CLASS_BITS[key] = (label2binlabel, out)
    return out


_UNIT_GRAD = {}
_UNIT_LEN = 64


def unit_gradient(device, n=1):
    """The library's constant all-ones float32 tensor of a device (``[n]``, ``n <= 64``: a prefix view of ONE
    cached buffer): a root gradient for ``total.backward(unit_gradient(dev))`` that is not refilled every step
    (``backward()`` without an argument launches a fill) and that the loss edges of this package RECOGNISE —
    :func:`gs_head_step`'s backward, the head's term split and ``train.parse_losses`` hand it on by identity, so
    that "every upstream factor is 1" is known on the host and the gradient the forward produced is the answer
    without a launch.  Recognition = same storage AND an untouched version counter: a tensor somebody wrote to
    in place (the buffer is an ordinary CUDA tensor) is NOT taken for ones — the general path runs."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    ent = _UNIT_GRAD.get(device)
    if ent is None or ent[0]._version != ent[1]:
        t = torch.ones(_UNIT_LEN, dtype=torch.float32, device=device)
        ent = _UNIT_GRAD[device] = (t, t._version)
    assert 1 <= n <= _UNIT_LEN
    return ent[0][:n]


def _is_unit_gradient(g):
    """``g`` is (a view of the head of) the cached all-ones buffer, and nobody has written to that buffer."""
    ent = _UNIT_GRAD.get(g.device)
    if ent is None or g.dtype != torch.float32:
        return False
    t, ver = ent
    return (t._version == ver and g.data_ptr() == t.data_ptr() and 1 <= g.numel() <= _UNIT_LEN
            and g.is_contiguous())


class _UnbindTermsFn(torch.autograd.Function):
    """``terms.unbind(0)`` for the fused head's loss vector with a backward that keeps the identity of unit
    gradients: when every term's upstream gradient IS the library's unit gradient (``loss.backward(
    unit_gradient(dev))`` through ``train.parse_losses``), the vector handed to the head's backward is the cached
    ones buffer itself — no stack launch, and the head launches nothing either.  Otherwise: one stack."""

    @staticmethod
    def forward(ctx, terms):
        ctx.n = terms.shape[0]
        ctx.set_materialize_grads(False)
        return tuple(terms.detach().unbind(0))

    @staticmethod
    def backward(ctx, *gs):
        if all(g is None for g in gs):
            return None
        if all(g is not None and g.numel() == 1 and _is_unit_gradient(g) for g in gs) and ctx.n <= _UNIT_LEN:
            return unit_gradient(gs[0].device, ctx.n)
        ref = next(g for g in gs if g is not None)
        return torch.stack([ref.new_zeros(()) if g is None else g.reshape(()) for g in gs])


def unbind_terms(terms):
    """The fused head's ``terms [B + 1]`` as B + 1 scalars (see :class:`_UnbindTermsFn`)."""
    return _UnbindTermsFn.apply(terms)


class _GsHeadStepFn(torch.autograd.Function):
    """``bgs_gs_head_step``: the whole ``GSBBoxHeadWith0.loss()`` as main kernel + reduce.  Returns
    ``terms [B + 1]`` = {per-bin losses (x loss weights), loss_bbox}, ``total [1]`` = their sum and
    ``avg [B]``; backward is ONE scaling launch over the gradients the forward already produced
    (early-out on the device when the upstream factors are 1), and NO launch when the upstream
    gradient of ``total`` is :func:`unit_gradient` itself."""

    @staticmethod
    def forward(ctx, logits, bbox_pred, labels, l2b, class_bits, pred_slice_host,
                bin_loss_weight_host, ratio, seed, counter, row_weights, bbox_targets, bbox_weights,
                num_reg_classes, beta, box_loss_weight, debug):
        import numpy as np
        lib = capi.load()
        z = _f32c(logits)
        N, W = z.shape
        B, C = l2b.shape
        dev = z.device
        box = bbox_pred is not None
        p = _f32c(bbox_pred) if box else None
        R = int(num_reg_classes) if box else 1
        if box:
            assert tuple(p.shape) == (N, 4 * R), (p.shape, N, R)
        terms = torch.empty((B + 1,), dtype=torch.float32, device=dev)
        total = torch.empty((1,), dtype=torch.float32, device=dev)
        avg = torch.empty((B,), dtype=torch.float32, device=dev)
        dlogits = torch.empty_like(z) if logits.requires_grad else None
        dbbox = torch.empty_like(p) if (box and bbox_pred.requires_grad) else None
        bl = torch.empty((B, N), dtype=torch.int32, device=dev) if debug else None
        w = torch.empty((B, N), dtype=torch.float32, device=dev) if debug else None
        ws = _workspace(lib.bgs_gs_loss_workspace_bytes(N, B), dev)
        ps_keep, ps_ptr = capi.host_i64(pred_slice_host)
        lw_keep = None if bin_loss_weight_host is None else \
            np.ascontiguousarray(bin_loss_weight_host, dtype=np.float32)
        lw_ptr = None if lw_keep is None else lw_keep.ctypes.data_as(ctypes.c_void_p)
        rw = None if row_weights is None else _f32c(row_weights)
        rc = lib.bgs_gs_head_step(
            capi.ptr(z), capi.ptr(labels), capi.ptr(l2b), capi.ptr(class_bits), capi.ptr(rw), ps_ptr,
            lw_ptr, N, C, B, W, float(ratio), int(seed), capi.ptr(counter), capi.ptr(p),
            capi.ptr(_f32c(bbox_targets)) if box else None,
            capi.ptr(_f32c(bbox_weights)) if box else None, R, float(beta), float(box_loss_weight),
            capi.ptr(terms), capi.ptr(total), capi.ptr(dlogits), capi.ptr(dbbox), capi.ptr(avg),
            capi.ptr(bl), capi.ptr(w), capi.ptr(ws), capi.current_stream(dev))
        capi.check('bgs_gs_head_step', rc)
        ctx.grads = (dlogits, dbbox)
        ctx.meta = (pred_slice_host, N, B, W, R, logits.dtype, None if not box else bbox_pred.dtype)
        ctx.consumed = False
        ctx.set_materialize_grads(False)     # an unused output (terms or total) arrives as None, not zeros
        if debug:
            ctx.mark_non_differentiable(avg, bl, w)
            return terms, total, avg, bl, w
        ctx.mark_non_differentiable(avg)
        return terms, total, avg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_terms, g_total, *_unused):
        dlogits, dbbox = ctx.grads
        ps_host, N, B, W, R, zdt, pdt = ctx.meta
        if (dlogits is None and dbbox is None) or (g_terms is None and g_total is None):
            return (None,) * 17
        if ctx.consumed:     # the buffers are scaled in place and handed to autograd (see _GroupSoftmaxLoss)
            raise RuntimeError('gs_head_step: the fused gradient buffers were consumed by the first '
                               'backward; call the loss again')
        if (g_terms is None and _is_unit_gradient(g_total)) or \
                (g_total is None and g_terms is not None and g_terms.numel() == B + 1 and _is_unit_gradient(g_terms)):
            pass          # the root gradient is the library's unit gradient, handed down by identity (directly to
            #               `total`, or to every term through parse_losses): every factor is 1 — no launch
        else:
            lib = capi.load()
            gt = None if g_terms is None else g_terms.detach().to(torch.float32).contiguous()
            gT = None if g_total is None else g_total.detach().to(torch.float32).contiguous()
            ps_keep, ps_ptr = capi.host_i64(ps_host)
            dev = (dlogits if dlogits is not None else dbbox).device
            rc = lib.bgs_gs_head_step_scale_grad(capi.ptr(dlogits), capi.ptr(dbbox), ps_ptr, capi.ptr(gt),
                                                 capi.ptr(gT), N, B, W, R, capi.current_stream(dev))
            capi.check('bgs_gs_head_step_scale_grad', rc)
        ctx.consumed = True
        ctx.grads = (None, None)      # sole owner now: AccumulateGrad can take the buffer instead of cloning it
        gz = dlogits if (dlogits is None or zdt == torch.float32) else dlogits.to(zdt)
        gp = dbbox if (dbbox is None or pdt == torch.float32) else dbbox.to(pdt)
        del dlogits, dbbox
        return (gz, gp) + (None,) * 15


def gs_head_step(cls_score, labels, label2binlabel, pred_slice, others_sample_ratio, seed,
                 draw_counter=None, row_weights=None, bin_loss_weight=None, bbox_pred=None,
                 bbox_targets=None, bbox_weights=None, num_reg_classes=1, beta=1.0,
                 box_loss_weight=1.0, debug=False, class_bits='auto'):
    """The whole BAGS head loss as two launches (``bgs_gs_head_step``): returns ``(terms, total,
    avg)`` with ``terms [B + 1]`` = per-bin classification losses (times ``bin_loss_weight``, a HOST
    sequence) followed by ``loss_bbox`` (0 without ``bbox_pred``), ``total [1]`` = their sum (both
    differentiable) and ``avg [B]``.  ``draw_counter``: device int64 ``[1]``, read as this call's
    draw index and advanced BY THE KERNEL (fresh "others" samples under hipGraph replay without a
    tensor op).  ``class_bits``: ``'auto'`` builds / reuses :func:`gs_class_bin_mask`, ``None`` lets
    every workgroup derive the table from ``label2binlabel``.  Limits of :func:`gs_head_loss_fused`."""
    _require_cuda(cls_score, labels, label2binlabel, row_weights, bbox_pred, bbox_targets,
                  bbox_weights, draw_counter)
    assert labels.dtype == torch.int64 and label2binlabel.dtype == torch.int64
    assert cls_score.dim() == 2 and 0 < cls_score.shape[0] <= GS_FUSED_MAX_ROWS
    if draw_counter is not None:
        assert draw_counter.dtype == torch.int64 and draw_counter.numel() == 1
    if bbox_pred is not None:
        assert bbox_targets is not None and bbox_weights is not None
    label2binlabel = label2binlabel.contiguous()
    if isinstance(class_bits, str):
        class_bits = gs_class_bin_mask(label2binlabel)
    return _GsHeadStepFn.apply(cls_score, bbox_pred, labels.contiguous(), label2binlabel, class_bits,
                               _host_pred_slice(pred_slice), bin_loss_weight,
                               float(others_sample_ratio), int(seed), draw_counter, row_weights,
                               bbox_targets, bbox_weights, int(num_reg_classes), float(beta),
                               float(box_loss_weight), bool(debug))


GS_FUSED_MAX_ROWS = 4096


def gs_head_loss_fused(cls_score, labels, label2binlabel, pred_slice, others_sample_ratio,
                       seed, seed_offset=None, row_weights=None, debug=False):
    """The BAGS head's classification loss straight from ``labels``: ``(losses [B], avg [B])``
    (``debug=True`` adds the bin labels and sample weights ``[B, N]`` the kernel used).
    Requires ``N <= 4096`` rows, ``B <= 15`` and no per-class reweighting; same values, bit for
    bit, as :func:`gs_prepare` + :func:`group_softmax_loss` with the same seed."""
    _require_cuda(cls_score, labels, label2binlabel, row_weights)
    assert labels.dtype == torch.int64 and label2binlabel.dtype == torch.int64
    assert cls_score.dim() == 2 and 0 < cls_score.shape[0] <= GS_FUSED_MAX_ROWS
    return _GsHeadFusedLoss.apply(cls_score, labels.contiguous(), label2binlabel.contiguous(),
                                  _host_pred_slice(pred_slice), float(others_sample_ratio), int(seed),
                                  seed_offset, row_weights, bool(debug))


def group_softmax_loss(cls_score, bin_labels, pred_slice, weights=None, avg=None):
    """Per-bin weighted CE of the ``[N, W]`` logits -> ``[B]`` losses (differentiable
    w.r.t. ``cls_score``).

    ``bin_labels [B,N] i32`` / ``weights [B,N]`` / ``avg [B]`` as produced by ``gs_prepare``;
    ``pred_slice``: HOST ``[B,2]`` (start, length) table (numpy / list / CPU tensor).
    """
    _require_cuda(cls_score, bin_labels, weights, avg)
    assert cls_score.dim() == 2 and bin_labels.dtype == torch.int32
    assert bin_labels.is_contiguous() and bin_labels.shape[1] == cls_score.shape[0]
    ps = _host_pred_slice(pred_slice)
    assert ps.shape == (bin_labels.shape[0], 2)
    if weights is not None:
        weights = _f32c(weights)
        assert weights.shape == tuple(bin_labels.shape)
    if avg is not None:
        avg = _f32c(avg)
    return _GroupSoftmaxLoss.apply(cls_score, bin_labels, ps, weights, avg)


def _host_pred_slice(pred_slice):
    import numpy as np
    if isinstance(pred_slice, torch.Tensor):
        if pred_slice.is_cuda:
            raise RuntimeError('pred_slice must live on the host (static metadata passed by '
                               'value to the kernels); keep a CPU copy instead of syncing')
        pred_slice = pred_slice.numpy()
    return np.ascontiguousarray(pred_slice, dtype=np.int64)


# ----------------------------------------------------------------------------------------
# inference score merge  (GSBBoxHeadWith0._merge_score, :239-273)
# ----------------------------------------------------------------------------------------
def gs_merge_score(cls_score, pred_slice, cls2col, num_classes):
    _require_cuda(cls_score, cls2col)
    lib = capi.load()
    z = _f32c(cls_score)
    N, W = z.shape
    ps_keep, ps_ptr = capi.host_i64(_host_pred_slice(pred_slice))
    B = ps_keep.shape[0]
    assert cls2col.dtype == torch.int32 and cls2col.numel() == num_classes
    out = torch.empty((N, num_classes), dtype=torch.float32, device=z.device)
    rc = lib.bgs_gs_merge_score(capi.ptr(z), ps_ptr, capi.ptr(cls2col), N,
                                num_classes, B, W, capi.ptr(out), capi.current_stream(z.device))
    capi.check('bgs_gs_merge_score', rc)
    return out


# ----------------------------------------------------------------------------------------
# tau-normalised two-head test  (tools/test_lvis_tnorm.py, test_mixins.py:70-92; csrc/tnorm.hip)
# ----------------------------------------------------------------------------------------
def _require_f32(name, **tensors):
    for arg, t in tensors.items():
        if t.dtype != torch.float32:
            raise NotImplementedError('%s: %s is %s; only float32 has a kernel' % (name, arg, t.dtype))


def _u8c(name, arg, t, n):
    """A mask / valid vector of ``n`` entries as contiguous uint8 (non-zero = set)."""
    if t.numel() != n:
        raise ValueError('%s: %s has %d entries, expected %d' % (name, arg, t.numel(), n))
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).view(torch.uint8)
    return t.reshape(-1).contiguous()


def tau_normalize(weight, tau, first_row=1):
    """``pnorm`` of ``reweight_cls_newhead`` (tools/test_lvis_tnorm.py:276-283): rows ``i >= first_row`` of
    ``weight [C, K]`` divided by ``||row||_2 ** tau``, the rows below copied -> a new ``[C, K]`` tensor.  One launch.
    A zero row gives NaN for ``tau > 0`` as in the reference; ``tau = 0`` returns the input bits."""
    _require_cuda(weight)
    _require_f32('tau_normalize', weight=weight)
    if weight.dim() != 2:
        raise ValueError('tau_normalize: weight must be [C, K], got %s' % (tuple(weight.shape),))
    if int(first_row) < 0:
        raise ValueError('tau_normalize: first_row must be >= 0')
    lib = capi.load()
    w = weight.detach().contiguous()
    C, K = w.shape
    out = torch.empty_like(w)
    if K > 0:
        rc = lib.bgs_tau_norm_rows(capi.ptr(w), C, K, int(first_row), float(tau), capi.ptr(out),
                                   capi.current_stream(w.device))
        capi.check('bgs_tau_norm_rows', rc)
    return out


def score_reweight_select(scores, scores_rw, mask, valid=None, out=None):
    """``BBoxTestMixin.update_scores_with_reweight`` (test_mixins.py:70-92) in one launch, no host read:
    a row whose chosen class (``argmax(scores)`` if that is the background, else ``argmax(scores_rw)``) is set in
    ``mask [C]`` takes the whole row of ``scores_rw`` -> ``(out [R, C], pred_label [R] int32)`` with
    ``pred_label = argmax(out, 1)`` (torch's CPU rule: first maximum, NaN counts as the maximum).
    ``valid [R]``: rows with ``valid == 0`` keep ``scores`` and get ``pred_label = -1``.  ``out``: the result tensor,
    which may be ``scores`` itself (the reference's in-place form); a fresh tensor by default."""
    _require_cuda(scores, scores_rw, mask, valid, out)
    _require_f32('score_reweight_select', scores=scores, scores_rw=scores_rw)
    if scores.dim() != 2 or tuple(scores.shape) != tuple(scores_rw.shape):
        raise ValueError('score_reweight_select: scores %s and scores_rw %s must be the same [R, C]'
                         % (tuple(scores.shape), tuple(scores_rw.shape)))
    R, C = scores.shape
    if C < 1:
        raise ValueError('score_reweight_select: no class column')
    m = _u8c('score_reweight_select', 'mask', mask, C)
    v = None if valid is None else _u8c('score_reweight_select', 'valid', valid, R)
    s = scores.detach()
    if out is None:
        s = s.contiguous()
        out = torch.empty_like(s)
    else:
        _require_f32('score_reweight_select', out=out)
        if tuple(out.shape) != (R, C) or not out.is_contiguous() or not s.is_contiguous():
            raise ValueError('score_reweight_select: out must be a contiguous [R, C] tensor (and scores contiguous)')
    q = scores_rw.detach().contiguous()
    if q.data_ptr() == out.data_ptr() and R:
        raise ValueError('score_reweight_select: out must not be scores_rw')
    pred = torch.empty((R,), dtype=torch.int32, device=s.device)
    rc = capi.load().bgs_score_reweight_select(capi.ptr(s), capi.ptr(q), capi.ptr(m), capi.ptr(v), R, C,
                                               capi.ptr(out), capi.ptr(pred), capi.current_stream(s.device))
    capi.check('bgs_score_reweight_select', rc)
    return out, pred


def cls_acc_count(pred_label, assigned_label, num_ins, num_get):
    """The counting loop of ``single_gpu_test`` (tools/test_lvis_tnorm.py:125-129) on device counters:
    ``num_ins[g] += 1`` and ``num_get[g] += (p == g)`` for every row with ``pred_label p >= 0`` and assigned label
    ``g`` in ``[0, C)``.  ``pred_label`` / ``assigned_label [R]`` int32, ``num_ins`` / ``num_get [C]`` int64,
    updated in place (integer atomics: exact whatever the order) and returned."""
    _require_cuda(pred_label, assigned_label, num_ins, num_get)
    for arg, t in (('pred_label', pred_label), ('assigned_label', assigned_label)):
        if t.dtype != torch.int32:
            raise NotImplementedError('cls_acc_count: %s is %s; int32 is what the kernel reads' % (arg, t.dtype))
    for arg, t in (('num_ins', num_ins), ('num_get', num_get)):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 1:
            raise ValueError('cls_acc_count: %s must be a contiguous int64 vector' % arg)
    if num_ins.numel() != num_get.numel() or pred_label.numel() != assigned_label.numel():
        raise ValueError('cls_acc_count: sizes differ')
    p, g = pred_label.reshape(-1).contiguous(), assigned_label.reshape(-1).contiguous()
    rc = capi.load().bgs_cls_acc_count(capi.ptr(p), capi.ptr(g), p.numel(), num_ins.numel(), capi.ptr(num_ins),
                                       capi.ptr(num_get), capi.current_stream(p.device))
    capi.check('bgs_cls_acc_count', rc)
    return num_ins, num_get


# ----------------------------------------------------------------------------------------
# NCM baseline  (mmdet/models/detectors/DCM.py; csrc/ncm.hip)
# ----------------------------------------------------------------------------------------
def class_sum_max_rows():
    """Rows one ``class_sum`` call takes (the labels of a call live in LDS)."""
    return int(capi.load().bgs_class_sum_max_rows())


def class_sum(fea, labels, sums, counts):
    """``sums[labels[g]] += fea[g]`` and ``counts[labels[g]] += 1`` in ascending ``g``, one rounded float64 add per
    row (bit-identical to ``np.add.at`` on float64; no atomics).  ``fea [G, D]`` float32, ``labels [G]`` int64,
    ``sums [C, D]`` float64 and ``counts [C]`` int64, both updated in place and returned.  Rows labelled outside
    ``[0, C)`` are skipped.  At most :func:`class_sum_max_rows` rows per call."""
    _require_cuda(fea, labels, sums, counts)
    _require_f32('class_sum', fea=fea)
    if labels.dtype != torch.int64:
        raise NotImplementedError('class_sum: labels is %s; int64 is what the kernel reads' % (labels.dtype,))
    if sums.dtype != torch.float64 or counts.dtype != torch.int64:
        raise NotImplementedError('class_sum: sums must be float64 and counts int64, got %s and %s'
                                  % (sums.dtype, counts.dtype))
    if fea.dim() != 2 or sums.dim() != 2 or fea.shape[1] != sums.shape[1] or fea.shape[1] < 1:
        raise ValueError('class_sum: fea %s and sums %s must be [G, D] and [C, D]'
                         % (tuple(fea.shape), tuple(sums.shape)))
    G, D = fea.shape
    C = sums.shape[0]
    if labels.dim() != 1 or labels.numel() != G or counts.dim() != 1 or counts.numel() != C:
        raise ValueError('class_sum: labels must be [%d] and counts [%d], got %s and %s'
                         % (G, C, tuple(labels.shape), tuple(counts.shape)))
    for arg, t in (('fea', fea), ('labels', labels), ('sums', sums), ('counts', counts)):
        if not t.is_contiguous():
            raise ValueError('class_sum: %s must be contiguous' % arg)
    rc = capi.load().bgs_class_sum(capi.ptr(fea.detach()), capi.ptr(labels), G, D, C, capi.ptr(sums), capi.ptr(counts),
                                   capi.current_stream(fea.device))
    capi.check('bgs_class_sum', rc)
    return sums, counts


def ncm_score(fea, unit_centres, cls_score, valid=None, out=None):
    """The scoring lines of ``DCM.simple_test_bboxes`` (DCM.py:192-203): one GEMM (:func:`linear`) and one launch.
    ``fea [R, D]``, ``unit_centres [C - 1, D]`` (the unit-norm foreground centres, ``ncm.load_centers``),
    ``cls_score [R, C]`` -> ``(out [R, C], pred_label [R] int32)`` with ``out[:, 0] = softmax(cls_score)[:, 0]``,
    ``out[:, 1:] = (1 - out[:, :1]) * softmax(cos(fea, centres))`` and ``pred_label = argmax(out, 1)`` (torch's CPU
    rule), -1 where ``valid [R]`` is 0.  ``out`` may be ``cls_score`` itself; a fresh tensor by default."""
    _require_cuda(fea, unit_centres, cls_score, valid, out)
    _require_f32('ncm_score', fea=fea, unit_centres=unit_centres, cls_score=cls_score)
    if fea.dim() != 2 or unit_centres.dim() != 2 or cls_score.dim() != 2:
        raise ValueError('ncm_score: fea, unit_centres and cls_score must be matrices')
    R, D = fea.shape
    C = cls_score.shape[1]
    if D < 1 or C < 2 or tuple(unit_centres.shape) != (C - 1, D) or cls_score.shape[0] != R:
        raise ValueError('ncm_score: fea %s, unit_centres %s and cls_score %s must be [R, D], [C - 1, D] and [R, C]'
                         % (tuple(fea.shape), tuple(unit_centres.shape), tuple(cls_score.shape)))
    for arg, t in (('fea', fea), ('unit_centres', unit_centres), ('cls_score', cls_score)):
        if not t.is_contiguous():
            raise ValueError('ncm_score: %s must be contiguous' % arg)
    v = None if valid is None else _u8c('ncm_score', 'valid', valid, R)
    f, s = fea.detach(), cls_score.detach()
    if out is None:
        out = torch.empty_like(s)
    else:
        _require_f32('ncm_score', out=out)
        if tuple(out.shape) != (R, C) or not out.is_contiguous():
            raise ValueError('ncm_score: out must be a contiguous [R, C] tensor')
    pred = torch.empty((R,), dtype=torch.int32, device=s.device)
    if R == 0:
        return out, pred
    fg, cg = f, unit_centres.detach()
    if D % 4 != 0:
        # the GEMM kernel reads K in 16-byte pieces: zero columns leave every dot product as it is (the norm below is
        # taken of the feature itself); the detector's widths (12544, 1024) never come here
        fg = torch.nn.functional.pad(fg, (0, 4 - D % 4))
        cg = torch.nn.functional.pad(cg, (0, 4 - D % 4))
    elif fg.data_ptr() % 16 != 0:
        fg = fg.clone()
    dots = linear(fg, cg, frozen_weight=D % 4 == 0 and not unit_centres.requires_grad)
    rc = capi.load().bgs_ncm_score(capi.ptr(f), capi.ptr(dots), capi.ptr(s), capi.ptr(v), R, D, C, capi.ptr(out),
                                   capi.ptr(pred), capi.current_stream(s.device))
    capi.check('bgs_ncm_score', rc)
    return out, pred


# ----------------------------------------------------------------------------------------
# box regression loss  (loss_bbox branch, :173-185)
# ----------------------------------------------------------------------------------------
class _BBoxSmoothL1(torch.autograd.Function):

    @staticmethod
    def forward(ctx, bbox_pred, labels, bbox_targets, bbox_weights, num_reg_classes, beta,
                avg_factor, loss_weight):
        lib = capi.load()
        p = _f32c(bbox_pred)
        N = p.shape[0]
        R = int(num_reg_classes)
        assert p.shape[1] == 4 * R
        dev = p.device
        want_grad = bbox_pred.requires_grad
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dpred = torch.empty_like(p) if want_grad else None
        ws = _workspace(lib.bgs_bbox_loss_workspace_bytes(N), dev)
        rc = lib.bgs_bbox_smooth_l1_fwd_bwd(
            capi.ptr(p), capi.ptr(labels), capi.ptr(bbox_targets), capi.ptr(bbox_weights), N, R,
            float(beta), float(avg_factor), float(loss_weight), capi.ptr(loss), capi.ptr(dpred),
            capi.ptr(ws), capi.current_stream(dev))
        capi.check('bgs_bbox_smooth_l1_fwd_bwd', rc)
        ctx.dpred = dpred
        ctx.in_dtype = bbox_pred.dtype
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        if ctx.dpred is None:
            return (None,) * 8
        g = ctx.dpred * grad_loss  # upstream scalar; dense like the autograd result
        if ctx.in_dtype != torch.float32:
            g = g.to(ctx.in_dtype)
        return (g,) + (None,) * 7


def bbox_smooth_l1_loss(bbox_pred, labels, bbox_targets, bbox_weights, num_reg_classes,
                        beta=1.0, avg_factor=None, loss_weight=1.0):
    """``loss_weight * sum(smooth_l1(pred[pos, labels[pos]] - targets[pos]) * w[pos]) / avg``."""
    _require_cuda(bbox_pred, labels, bbox_targets, bbox_weights)
    if avg_factor is None:
        avg_factor = bbox_targets.shape[0]
    return _BBoxSmoothL1.apply(bbox_pred, labels.contiguous(), _f32c(bbox_targets),
                               _f32c(bbox_weights), num_reg_classes, beta, avg_factor,
                               loss_weight)


class _BBoxBalancedL1(torch.autograd.Function):

    @staticmethod
    def forward(ctx, bbox_pred, labels, bbox_targets, bbox_weights, num_reg_classes, alpha, gamma, beta,
                avg_factor, loss_weight):
        lib = capi.load()
        p = _f32c(bbox_pred)
        N = p.shape[0]
        R = int(num_reg_classes)
        assert p.shape[1] == 4 * R
        dev = p.device
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dpred = torch.empty_like(p) if bbox_pred.requires_grad else None
        ws = _workspace(lib.bgs_bbox_loss_workspace_bytes(N), dev)
        rc = lib.bgs_bbox_balanced_l1_fwd_bwd(
            capi.ptr(p), capi.ptr(labels), capi.ptr(bbox_targets), capi.ptr(bbox_weights), N, R,
            float(alpha), float(gamma), float(beta), float(avg_factor), float(loss_weight), capi.ptr(loss),
            capi.ptr(dpred), capi.ptr(ws), capi.current_stream(dev))
        capi.check('bgs_bbox_balanced_l1_fwd_bwd', rc)
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        if ctx.dpred is None:
            return (None,) * 10
        return (ctx.dpred * grad_loss,) + (None,) * 9


def bbox_balanced_l1_loss(bbox_pred, labels, bbox_targets, bbox_weights, num_reg_classes,
                          alpha=0.5, gamma=1.5, beta=1.0, avg_factor=None, loss_weight=1.0):
    """``loss_weight * sum(balanced_l1(pred[pos, labels[pos]] - targets[pos]) * w[pos]) / avg``
    (mmdet/models/losses/balanced_l1_loss.py:19-24): :func:`bbox_smooth_l1_loss` with the other element loss."""
    _require_cuda(bbox_pred, labels, bbox_targets, bbox_weights)
    _require_f32('bbox_balanced_l1_loss', bbox_pred=bbox_pred, bbox_targets=bbox_targets, bbox_weights=bbox_weights)
    if not (alpha > 0 and gamma > 0 and beta > 0):
        raise ValueError('bbox_balanced_l1_loss: alpha, gamma and beta must be > 0')
    if avg_factor is None:
        avg_factor = bbox_targets.shape[0]
    return _BBoxBalancedL1.apply(bbox_pred, labels.contiguous(), _f32c(bbox_targets), _f32c(bbox_weights),
                                 num_reg_classes, alpha, gamma, beta, avg_factor, loss_weight)


# ----------------------------------------------------------------------------------------
# balanced feature pyramid: gather and scatter  (mmdet/models/necks/bfp.py:74-100; csrc/bfp.hip)
# ----------------------------------------------------------------------------------------
def _bfp_levels(name, inputs, refine_level):
    """Checked pyramid -> (list of contiguous fp32 NHWC levels, host ``[L, 2]`` int size table, B, C)."""
    inputs = list(inputs)
    L = len(inputs)
    if L < 1:
        raise ValueError('%s: no levels' % name)
    if L > capi.BGS_BFP_MAX_LEVELS:
        raise NotImplementedError('%s: %d levels; the level table of the kernels holds at most %d (num_levels)'
                                  % (name, L, capi.BGS_BFP_MAX_LEVELS))
    if not 0 <= refine_level < L:
        raise ValueError('%s: refine_level %d outside [0, %d)' % (name, refine_level, L))
    if inputs[0].dim() != 4:
        raise ValueError('%s: level 0 is %s; every level is NHWC [B, H, W, C]' % (name, tuple(inputs[0].shape)))
    B, C = inputs[0].shape[0], inputs[0].shape[3]
    for i, t in enumerate(inputs):
        if t.dim() != 4 or t.shape[0] != B or t.shape[3] != C:
            raise ValueError('%s: level %d is %s; every level is NHWC [%d, H, W, %d]' % (name, i, tuple(t.shape), B, C))
    if C % 4 != 0:
        raise NotImplementedError('%s: C %% 4 != 0 (C = %d); a thread owns 4 channels (16-byte accesses)' % (name, C))
    _require_cuda(*inputs)
    _require_f32(name, **{'level_%d' % i: t for i, t in enumerate(inputs)})
    hw = (ctypes.c_int * (2 * L))(*[int(v) for t in inputs for v in t.shape[1:3]])
    return inputs, hw, B, C


def _ptr_table(tensors):
    """Host array of device pointers (``None`` -> NULL) for the ``host_*`` parameters of the BFP kernels."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _c16(t):
    """Detached, contiguous, 16-byte aligned."""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _BfpGather(torch.autograd.Function):
    """``(x_0 .. x_{L-1}) -> (bsf, x_0 .. x_{L-1})``: the levels pass through the node unchanged, so that the gradients
    the scatter's residual path sends to them arrive HERE and ``bgs_bfp_gather_bwd`` adds each level's own share of
    ``d bsf`` to them in its one launch (no accumulation launches per level)."""

    @staticmethod
    def forward(ctx, refine_level, want, *xs):
        xs_c, hw, B, C = _bfp_levels('bfp_gather', xs, refine_level)
        ctx.set_materialize_grads(False)      # a level nobody sent a gradient to reaches the kernel as NULL, not as zeros
        xs_c = [_c16(t) for t in xs_c]
        L = len(xs_c)
        hr, wr = xs_c[refine_level].shape[1:3]
        dev = xs_c[0].device
        bsf = torch.empty((B, hr, wr, C), dtype=torch.float32, device=dev)
        idx = [torch.empty((B, hr, wr, C), dtype=torch.int32, device=dev) if want and i < refine_level else None
               for i in range(L)]
        rc = capi.load().bgs_bfp_gather(_ptr_table(xs_c), hw, L, refine_level, B, C, capi.ptr(bsf),
                                        _ptr_table(idx) if want else None, capi.current_stream(dev))
        capi.check('bgs_bfp_gather', rc)
        ctx.geom = (hw, L, refine_level, B, C, [tuple(t.shape) for t in xs_c])
        ctx.idx = idx
        return (bsf,) + tuple(xs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *douts):
        hw, L, refine_level, B, C, shapes = ctx.geom
        if g is None:                         # bsf went nowhere: the levels' gradients pass by identity
            return (None, None) + tuple(douts)
        dev = g.device
        g = _c16(g)
        douts = [None if d is None else _c16(d) for d in douts]
        dxs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        rc = capi.load().bgs_bfp_gather_bwd(capi.ptr(g), _ptr_table(douts), _ptr_table(ctx.idx), hw, L, refine_level,
                                            B, C, _ptr_table(dxs), capi.current_stream(dev))
        capi.check('bgs_bfp_gather_bwd', rc)
        return (None, None) + tuple(dxs)


class _BfpScatter(torch.autograd.Function):

    @staticmethod
    def forward(ctx, refine_level, want, bsf, *xs):
        xs_c, hw, B, C = _bfp_levels('bfp_scatter', xs, refine_level)
        _require_cuda(bsf)
        _require_f32('bfp_scatter', bsf=bsf)
        if tuple(bsf.shape) != tuple(xs_c[refine_level].shape):
            raise ValueError('bfp_scatter: bsf is %s, the refine level %s' % (tuple(bsf.shape),
                                                                               tuple(xs_c[refine_level].shape)))
        xs_c = [_c16(t) for t in xs_c]
        bsf_c = _c16(bsf)
        L = len(xs_c)
        dev = bsf_c.device
        outs = [torch.empty_like(t) for t in xs_c]
        idx = [torch.empty(t.shape, dtype=torch.int32, device=dev) if want and i >= refine_level else None
               for i, t in enumerate(xs_c)]
        rc = capi.load().bgs_bfp_scatter(capi.ptr(bsf_c), _ptr_table(xs_c), hw, L, refine_level, B, C,
                                         _ptr_table(outs), _ptr_table(idx) if want else None,
                                         capi.current_stream(dev))
        capi.check('bgs_bfp_scatter', rc)
        ctx.geom = (hw, L, refine_level, B, C, tuple(bsf_c.shape))
        ctx.idx = idx
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        hw, L, refine_level, B, C, shape = ctx.geom
        d_bsf = None
        if ctx.needs_input_grad[2]:
            dc = [_c16(d) for d in douts]
            d_bsf = torch.empty(shape, dtype=torch.float32, device=dc[0].device)
            rc = capi.load().bgs_bfp_scatter_bwd(_ptr_table(dc), _ptr_table(ctx.idx), hw, L, refine_level, B, C,
                                                 capi.ptr(d_bsf), capi.current_stream(d_bsf.device))
            capi.check('bgs_bfp_scatter_bwd', rc)
        # d x_i = dout_i: the residual path is the identity
        return (None, None, d_bsf) + tuple(d if need else None for d, need in zip(douts, ctx.needs_input_grad[3:]))


def bfp_gather(inputs, refine_level):
    """BFP step 1 (bfp.py:74-86) in one launch: ``bsf = (((0 + r_0) + r_1) + ...) / L`` with ``r_i`` the adaptive max
    pool (``i < refine_level``) or nearest resize (``i >= refine_level``) of level ``i`` to the refine level's size.
    fp32 NHWC levels -> ``(bsf, levels)``: hand THESE ``levels`` to :func:`bfp_scatter` — under autograd they are the
    inputs routed through the gather's node (same storage), which lets one backward launch add the residual path's
    gradient and the gather's own; without gradients they are the inputs and no index buffer is allocated."""
    want = torch.is_grad_enabled() and any(t.requires_grad for t in inputs)   # (arg-max buffers only then)
    res = _BfpGather.apply(int(refine_level), want, *inputs)
    return res[0], tuple(res[1:])


def bfp_scatter(bsf, inputs, refine_level):
    """BFP step 3 (bfp.py:92-100) in one launch: ``out_i = resize_i(bsf) + x_i``, nearest for ``i < refine_level``,
    adaptive max pool for ``i >= refine_level``.  -> tuple of fp32 NHWC levels."""
    want = torch.is_grad_enabled() and bsf.requires_grad
    return _BfpScatter.apply(int(refine_level), want, bsf, *inputs)


# ----------------------------------------------------------------------------------------
# NonLocal2D attention core  (mmdet/models/plugins/non_local.py:74-81, 103-108; csrc/non_local.hip)
# ----------------------------------------------------------------------------------------
NON_LOCAL_CHANNELS = (32, 64, 128, 256)


def _nl_rows(t):
    """``t [B, ..., Ci]`` as a ``[B, N, Ci]`` view with strides ``(N * ld, ld, 1)`` and a 16-byte aligned start, or None
    where no such view exists (the caller copies)."""
    v = t.detach()
    B, ci = v.shape[0], v.shape[-1]
    n = v.numel() // max(B * ci, 1)
    try:
        v = v.view(B, n, ci)
    except RuntimeError:
        return None
    # (one position per image: the row stride is free, so it is taken to be the image stride)
    ld = v.stride(1) if n > 1 else (v.stride(0) if B > 1 else ci)
    ok = v.stride(2) == 1 and ld >= ci and ld % 4 == 0 and (B == 1 or v.stride(0) == n * ld) and \
        v.data_ptr() % 16 == 0
    if not ok:
        return None
    return v if v.stride(1) == ld else v.as_strided((B, n, ci), (n * ld, ld, 1))


def _nl_check(name, theta, phi, g):
    if theta.dim() < 3 or theta.shape != phi.shape or theta.shape != g.shape:
        raise ValueError('%s: theta, phi and g must share one shape [B, N, Ci] or [B, H, W, Ci], got %s, %s, %s'
                         % (name, tuple(theta.shape), tuple(phi.shape), tuple(g.shape)))
    _require_f32(name, theta=theta, phi=phi, g=g)
    ci = theta.shape[-1]
    if ci not in NON_LOCAL_CHANNELS:
        raise NotImplementedError('%s: Ci = %d (inter_channels); the kernels are built for Ci in %s'
                                  % (name, ci, list(NON_LOCAL_CHANNELS)))
    _require_cuda(theta, phi, g)
    if theta.numel() == 0:
        raise ValueError('%s: empty input %s' % (name, tuple(theta.shape)))
    if theta.numel() >= 2 ** 31:
        raise NotImplementedError('%s: B * N * Ci >= 2^31 (32-bit indexing)' % name)
    if theta.shape[0] > 65535:
        raise NotImplementedError('%s: B = %d > 65535' % (name, theta.shape[0]))


def _nl_forward(theta, phi, g, scale):
    """-> (y [B, N, Ci], ml [B, N, 2] = row maximum and sum, the three [B, N, Ci] views the kernel read, their row
    stride)"""
    views = [_nl_rows(t) for t in (theta, phi, g)]
    if any(v is None for v in views) or len(set(v.stride(1) for v in views)) != 1:
        B, ci = theta.shape[0], theta.shape[-1]
        views = [_c16(t).view(B, -1, ci) for t in (theta, phi, g)]
    th, ph, gg = views
    B, N, ci = th.shape
    ld = th.stride(1)               # (_nl_rows and the contiguous copies both leave (N * ld, ld, 1))
    assert ld >= ci and all(v.stride() == (N * ld, ld, 1) or B == 1 and v.stride()[1:] == (ld, 1) for v in views)
    y = torch.empty((B, N, ci), dtype=torch.float32, device=th.device)
    ml = torch.empty((B, N, 2), dtype=torch.float32, device=th.device)
    rc = capi.load().bgs_non_local_fwd(capi.ptr(th), capi.ptr(ph), capi.ptr(gg), ld, B, N, ci, scale, capi.ptr(y),
                                       None, capi.ptr(ml), capi.current_stream(th.device))
    capi.check('bgs_non_local_fwd', rc)
    return y, ml, views, ld


def _nl_backward(dy, y, ml, views, ld, scale, outs, ldd):
    th, ph, gg = views
    B, N, ci = th.shape
    dy = _c16(dy).view(B, N, ci)
    delta = torch.empty((B, N), dtype=torch.float32, device=dy.device)
    rc = capi.load().bgs_non_local_bwd(capi.ptr(dy), capi.ptr(y), capi.ptr(ml), capi.ptr(th), capi.ptr(ph),
                                       capi.ptr(gg), ld, B, N, ci, scale, capi.ptr(outs[0]), capi.ptr(outs[1]),
                                       capi.ptr(outs[2]), ldd, capi.ptr(delta), capi.current_stream(dy.device))
    capi.check('bgs_non_local_bwd', rc)


class _NonLocalFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, theta, phi, g, scale):
        y, ml, views, ld = _nl_forward(theta, phi, g, scale)
        if any(ctx.needs_input_grad[:3]):
            # (views of the inputs' storage, or the copies the kernel read: kept by reference, as _ConvFn keeps x)
            ctx.kept = (y, ml, views, ld, scale, tuple(theta.shape))
        return y.view(theta.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, ml, views, ld, scale, shape = ctx.kept
        B, N, ci = y.shape
        outs = [torch.empty((B, N, ci), dtype=torch.float32, device=y.device) for _ in range(3)]
        _nl_backward(dy, y, ml, views, ld, scale, outs, ci)
        return tuple(o.view(shape) if need else None for o, need in zip(outs, ctx.needs_input_grad[:3])) + (None,)


class _NonLocalPackedFn(torch.autograd.Function):
    """``tpg [B, ..., 3 * Ci]`` = theta | phi | g side by side (the output of one conv on the concatenated filter):
    the kernels read the three column slices in place and the backward writes the three gradients into the column
    slices of ONE ``[B, ..., 3 * Ci]`` tensor, which is the gradient of ``tpg`` — no slicing nodes, no concatenation."""

    @staticmethod
    def forward(ctx, tpg, scale):
        ci = tpg.shape[-1] // 3
        t = _c16(tpg)
        y, ml, views, ld = _nl_forward(t[..., :ci], t[..., ci:2 * ci], t[..., 2 * ci:], scale)
        if ctx.needs_input_grad[0]:
            ctx.kept = (y, ml, views, ld, scale, tuple(tpg.shape))
        return y.view(tuple(tpg.shape[:-1]) + (ci,))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, ml, views, ld, scale, shape = ctx.kept
        ci = y.shape[2]
        d = torch.empty(shape, dtype=torch.float32, device=y.device)
        _nl_backward(dy, y, ml, views, ld, scale, [d[..., :ci], d[..., ci:2 * ci], d[..., 2 * ci:]], 3 * ci)
        return d, None


def non_local_scale(inter_channels, use_scale=True):
    """The ``scale`` of :func:`non_local_attention` for ``NonLocal2D(use_scale=...)`` (non_local.py:77-79):
    ``1 / sqrt(Ci)`` computed in double (rounded to float once, where the launch takes it), or 1."""
    return 1.0 / math.sqrt(inter_channels) if use_scale else 1.0


def non_local_attention(theta, phi, g, scale):
    """``y[b, i, :] = sum_j softmax_j(scale * <theta[b, i, :], phi[b, j, :]>) * g[b, j, :]``: the attention core of
    ``NonLocal2D`` (non_local.py:74-81, 103-108, mode ``'embedded_gaussian'``) as ONE streaming launch, with an
    autograd node (two launches, no atomics).  No ``[N, N]`` matrix is ever written.  fp32 ``[B, N, Ci]`` or
    ``[B, H, W, Ci]`` (NHWC is already ``[N, Ci]`` row-major), ``Ci`` in ``NON_LOCAL_CHANNELS``; column slices of one
    ``[B, H, W, 3 * Ci]`` tensor are read in place.  ``scale``: a Python float (:func:`non_local_scale`)."""
    _nl_check('non_local_attention', theta, phi, g)
    return _NonLocalFn.apply(theta, phi, g, float(scale))


def non_local_attention_packed(tpg, scale):
    """:func:`non_local_attention` on ``theta | phi | g`` packed along the last axis of one fp32 tensor
    ``[B, ..., 3 * Ci]``; its gradient is one tensor of the same shape, written in place by the backward launches."""
    if tpg.dim() < 3 or tpg.shape[-1] % 3 != 0:
        raise ValueError('non_local_attention_packed: expected [B, ..., 3 * Ci], got %s' % (tuple(tpg.shape),))
    ci = tpg.shape[-1] // 3
    _nl_check('non_local_attention_packed', tpg[..., :ci], tpg[..., ci:2 * ci], tpg[..., 2 * ci:])
    return _NonLocalPackedFn.apply(tpg, float(scale))


# ----------------------------------------------------------------------------------------
# GCNet global-context block  (mmdet/ops/context_block.py; csrc/context_block.hip)
# ----------------------------------------------------------------------------------------
GC_MAX_CHANNELS = 2048
GC_EPS = 1e-5           # nn.LayerNorm's default, which the reference's block uses


def _gc_dims(name, x):
    """Checked fp32 ``[B, N, C]`` / ``[B, H, W, C]`` map -> ``(B, N, C)``."""
    if x.dim() not in (3, 4):
        raise ValueError('%s: x is %s; expected NHWC [B, H, W, C] or [B, N, C]' % (name, tuple(x.shape)))
    _require_f32(name, x=x)
    C = x.shape[-1]
    if C % 4 != 0:
        raise NotImplementedError('%s: C %% 4 != 0 (C = %d); a thread owns 4 channels (16-byte accesses)' % (name, C))
    if C > GC_MAX_CHANNELS:
        raise NotImplementedError('%s: C > %d (C = %d); a wave keeps one row of x in registers'
                                  % (name, GC_MAX_CHANNELS, C))
    _require_cuda(x)
    if x.numel() == 0:
        raise ValueError('%s: empty input %s' % (name, tuple(x.shape)))
    B = x.shape[0]
    return B, x.numel() // (B * C), C


def _gc_vec(name, arg, t, n):
    """A parameter or per-image vector of ``n`` floats, detached, contiguous and 16-byte aligned (or None)."""
    if t is None:
        return None
    _require_f32(name, **{arg: t})
    _require_cuda(t)
    if t.numel() != n:
        raise ValueError('%s: %s is %s, expected %d values' % (name, arg, tuple(t.shape), n))
    return _c16(t)


def _gc_branch(name, arg, br, C):
    """The six tensors of a ``channel_*_conv`` (conv weight and bias, LayerNorm weight and bias, conv weight and bias; the
    ``[P, C, 1, 1]`` filters are read in place as ``[P, C]``) -> (list of contiguous tensors or None, P)."""
    if br is None:
        return None, 0
    br = list(br)
    if len(br) != 6 or br[0].dim() < 2:
        raise ValueError('%s: %s must be (W1 [P, C], b1, ln_weight, ln_bias, W2 [C, P], b2)' % (name, arg))
    P = br[0].shape[0]
    sizes = (P * C, P, P, P, C * P, C)
    return [_gc_vec(name, '%s[%d]' % (arg, i), t, n) for i, (t, n) in enumerate(zip(br, sizes))], P


def _gc_planes(name, add, mul):
    if add[0] is not None and mul[0] is not None and add[1] != mul[1]:
        raise ValueError('%s: the add branch has %d planes, the mul branch %d' % (name, add[1], mul[1]))
    return (add if add[0] is not None else mul)[1]


def _gc_pool_launch(x, B, N, C, w_mask, b_mask, splits=None):
    """-> (part [B, S, C], part_ml [B, S, 2], s [B, N] or None, S)"""
    lib, dev = capi.load(), x.device
    S = int(splits) if splits is not None else lib.bgs_gc_num_splits(B, N)
    part = torch.empty((B, S, C), dtype=torch.float32, device=dev)
    part_ml = torch.empty((B, S, 2), dtype=torch.float32, device=dev)
    s = torch.empty((B, N), dtype=torch.float32, device=dev) if w_mask is not None else None
    rc = lib.bgs_gc_pool_fwd(capi.ptr(x), capi.ptr(w_mask), capi.ptr(b_mask), B, N, C, S, capi.ptr(s), capi.ptr(part),
                             capi.ptr(part_ml), capi.current_stream(dev))
    capi.check('bgs_gc_pool_fwd', rc)
    return part, part_ml, s, S


def _gc_channel_launch(part, part_ml, S, B, C, P, add, mul, eps):
    """-> (ctx [B, C], ml [B, 2], add term, mul term, hn_add, hn_mul, rstd)"""
    dev = part.device

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    ctx, ml = new(B, C), new(B, 2)
    t_add, hn_add = (new(B, C), new(B, 2, P)) if add is not None else (None, None)
    t_mul, hn_mul = (new(B, C), new(B, 2, P)) if mul is not None else (None, None)
    rstd = new(B, 2) if (add is not None or mul is not None) else None
    rc = capi.load().bgs_gc_channel_fwd(
        capi.ptr(part), capi.ptr(part_ml), S, B, C, P, None if add is None else _ptr_table(add),
        None if mul is None else _ptr_table(mul), eps, capi.ptr(ctx), capi.ptr(ml), capi.ptr(t_add), capi.ptr(t_mul),
        capi.ptr(hn_add), capi.ptr(hn_mul), capi.ptr(rstd), capi.current_stream(dev))
    capi.check('bgs_gc_channel_fwd', rc)
    return ctx, ml, t_add, t_mul, hn_add, hn_mul, rstd


def _gc_apply_launch(x, B, N, C, t_mul, t_add, identity, relu):
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    rc = capi.load().bgs_gc_apply_fwd(capi.ptr(x), capi.ptr(t_mul), capi.ptr(t_add), capi.ptr(identity), int(bool(relu)),
                                      B, N, C, capi.ptr(y), capi.current_stream(x.device))
    capi.check('bgs_gc_apply_fwd', rc)
    return y


def gc_pool(x, w_mask=None, b_mask=None, splits=None):
    """``spatial_pool`` of the reference's ``ContextBlock`` (context_block.py:64-88) on an fp32 NHWC map:
    ``ctx[b, c] = sum_n softmax_n(<x_n, w_mask> + b_mask) x[b, n, c]`` (``'att'``), or the mean over the positions when
    ``w_mask`` is None (``'avg'``).  -> ``(ctx [B, C], s [B, N] logits or None, ml [B, 2] = maximum and sum of
    exp(s - maximum))``.  One pass over ``x`` (a row is read once) leaves per-split partials, a second small launch
    combines them in split order.  Forward only: the differentiable form is :func:`context_block_nhwc`."""
    B, N, C = _gc_dims('gc_pool', x)
    w_mask = _gc_vec('gc_pool', 'w_mask', w_mask, C)
    b_mask = _gc_vec('gc_pool', 'b_mask', b_mask, 1)
    part, part_ml, s, S = _gc_pool_launch(_c16(x), B, N, C, w_mask, b_mask, splits)
    ctx, ml = _gc_channel_launch(part, part_ml, S, B, C, 0, None, None, GC_EPS)[:2]
    return ctx, s, ml


def gc_channel(ctx, add=None, mul=None, eps=GC_EPS):
    """``channel_add_conv`` / ``channel_mul_conv`` (context_block.py:36-51, 95-102) on ``ctx [B, C]``, both branches and
    all images in one launch: ``W2 relu(LayerNorm(W1 ctx + b1)) + b2`` (biased variance, ``eps``), a sigmoid on the
    ``mul`` branch.  ``add`` / ``mul``: the six tensors of a branch or None.  -> ``(add term, mul term)`` ``[B, C]``."""
    if ctx.dim() != 2:
        raise ValueError('gc_channel: ctx is %s; expected [B, C]' % (tuple(ctx.shape),))
    B, _, C = _gc_dims('gc_channel', ctx.unsqueeze(1))
    if add is None and mul is None:
        raise ValueError('gc_channel: neither an add nor a mul branch')
    add, mul = _gc_branch('gc_channel', 'add', add, C), _gc_branch('gc_channel', 'mul', mul, C)
    P = _gc_planes('gc_channel', add, mul)
    return _gc_channel_launch(_c16(ctx), None, 1, B, C, P, add[0], mul[0], float(eps))[2:4]


def gc_apply(x, mul=None, add=None, identity=None, relu=False):
    """``y = relu?(x * mul[b, c] + add[b, c] + identity)`` in one pass: the block's fusion (context_block.py:94-102) and
    the bottleneck's ``out += identity; relu`` (resnet.py:255, 264).  ``mul`` / ``add`` ``[B, C]`` and ``identity``
    (shaped like ``x``) are each optional.  Forward only."""
    B, N, C = _gc_dims('gc_apply', x)
    mul, add = _gc_vec('gc_apply', 'mul', mul, B * C), _gc_vec('gc_apply', 'add', add, B * C)
    identity = _gc_vec('gc_apply', 'identity', identity, x.numel())
    return _gc_apply_launch(_c16(x), B, N, C, mul, add, identity, relu)


def _gc_forward(x, w_mask, b_mask, add, mul, identity, relu, eps):
    """The three forward launches on checked, contiguous tensors -> (y, what the backward reads)."""
    B, N, C = x.shape[0], x.numel() // (x.shape[0] * x.shape[-1]), x.shape[-1]
    P = (add if add is not None else mul)[0].shape[0]
    part, part_ml, s, S = _gc_pool_launch(x, B, N, C, w_mask, b_mask)
    ctx, ml, t_add, t_mul, hn_add, hn_mul, rstd = _gc_channel_launch(part, part_ml, S, B, C, P, add, mul, eps)
    y = _gc_apply_launch(x, B, N, C, t_mul, t_add, identity, relu)
    return y, (B, N, C, P, S, s, ml, ctx, t_mul, hn_add, hn_mul, rstd)


class _ContextBlockFn(torch.autograd.Function):
    """The whole block as one node: three launches forward, four backward (two passes over the map)."""

    @staticmethod
    def forward(ctx, x, identity, relu, eps, w_mask, b_mask, *branches):
        add = None if branches[0] is None else [_c16(t) for t in branches[:6]]
        mul = None if branches[6] is None else [_c16(t) for t in branches[6:]]
        xc = _c16(x)
        wm = None if w_mask is None else _c16(w_mask)
        bm = None if b_mask is None else _c16(b_mask)
        y, kept = _gc_forward(xc, wm, bm, add, mul, None if identity is None else _c16(identity), relu, eps)
        ctx.kept = (xc, y if relu else None, wm, add, mul, relu, identity is not None) + kept
        ctx.shapes = [None if t is None else tuple(t.shape) for t in (w_mask, b_mask) + tuple(branches)]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, wm, add, mul, relu, has_id, B, N, C, P, S, s, ml, cx, t_mul, hn_add, hn_mul, rstd = ctx.kept
        lib, dev = capi.load(), x.device
        st = capi.current_stream(dev)

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        dy = _c16(dy)
        g = torch.empty_like(dy) if relu else dy
        part_a, part_m = new(B, S, C), (new(B, S, C) if mul is not None else None)
        rc = lib.bgs_gc_colsum_bwd(capi.ptr(dy), capi.ptr(y), capi.ptr(x) if mul is not None else None, B, N, C, S,
                                   capi.ptr(g) if relu else None, capi.ptr(part_a), capi.ptr(part_m), st)
        capi.check('bgs_gc_colsum_bwd', rc)
        dpre_a, dhz_a = (new(B, C), new(B, 2, P)) if add is not None else (None, None)
        dpre_m, dhz_m = (new(B, C), new(B, 2, P)) if mul is not None else (None, None)
        dctx = new(B, C)
        rc = lib.bgs_gc_channel_bwd(capi.ptr(part_a), capi.ptr(part_m), S, B, C, P,
                                    None if add is None else _ptr_table(add), None if mul is None else _ptr_table(mul),
                                    capi.ptr(t_mul), capi.ptr(hn_add), capi.ptr(hn_mul), capi.ptr(rstd),
                                    capi.ptr(dpre_a), capi.ptr(dpre_m), capi.ptr(dhz_a), capi.ptr(dhz_m),
                                    capi.ptr(dctx), st)
        capi.check('bgs_gc_channel_bwd', rc)
        dx = torch.empty_like(x)
        part_dw, part_ds = (new(B, S, C), new(B, S)) if wm is not None else (None, None)
        rc = lib.bgs_gc_dx_bwd(capi.ptr(g), capi.ptr(x), capi.ptr(s), capi.ptr(ml), capi.ptr(cx), capi.ptr(dctx),
                               capi.ptr(t_mul), capi.ptr(wm), B, N, C, S, capi.ptr(dx), capi.ptr(part_dw),
                               capi.ptr(part_ds), st)
        capi.check('bgs_gc_dx_bwd', rc)
        sizes = (P * C, P, P, P, C * P, C)
        d_add = [new(n) for n in sizes] if add is not None else None
        d_mul = [new(n) for n in sizes] if mul is not None else None
        dw_mask, db_mask = (new(C), new(1)) if wm is not None else (None, None)
        rc = lib.bgs_gc_param_bwd(B, S, C, P, capi.ptr(cx), capi.ptr(dpre_a), capi.ptr(dpre_m), capi.ptr(hn_add),
                                  capi.ptr(hn_mul), capi.ptr(dhz_a), capi.ptr(dhz_m), capi.ptr(part_dw),
                                  capi.ptr(part_ds), None if d_add is None else _ptr_table(d_add),
                                  None if d_mul is None else _ptr_table(d_mul), capi.ptr(dw_mask), capi.ptr(db_mask), st)
        capi.check('bgs_gc_param_bwd', rc)
        grads = [dw_mask, db_mask] + (d_add or [None] * 6) + (d_mul or [None] * 6)
        grads = [None if (t is None or not need) else t.view(shape)
                 for t, shape, need in zip(grads, ctx.shapes, ctx.needs_input_grad[4:])]
        return (dx if ctx.needs_input_grad[0] else None, g if has_id and ctx.needs_input_grad[1] else None,
                None, None) + tuple(grads)


def context_block_nhwc(x, params, identity=None, relu=False):
    """The reference's ``ContextBlock.forward`` (context_block.py:90-104) on an fp32 NHWC map, optionally followed by the
    bottleneck's ``out += identity`` and ReLU (resnet.py:255, 264), as ONE autograd node: three launches forward (pool,
    channel MLPs, apply), four backward.  ``params``: dict with ``w_mask`` / ``b_mask`` (``conv_mask``'s weight and bias;
    ``w_mask`` None selects ``pooling_type='avg'``), ``add`` / ``mul`` (the six tensors of ``channel_add_conv`` /
    ``channel_mul_conv``: conv, LayerNorm, conv; None for an absent branch) and optionally ``eps``.  With ``relu`` the
    result is an ordinary ReLU output whose gate this node's backward applies."""
    name = 'context_block_nhwc'
    if params.get('add') is None and params.get('mul') is None:
        raise ValueError('%s: neither an add nor a mul branch' % name)
    B, N, C = _gc_dims(name, x)
    w_mask, b_mask = params.get('w_mask'), params.get('b_mask')
    if w_mask is not None and b_mask is None:
        raise ValueError('%s: w_mask without b_mask' % name)
    if w_mask is None:
        b_mask = None
    _gc_vec(name, 'w_mask', w_mask, C)
    _gc_vec(name, 'b_mask', b_mask, 1)
    add, mul = _gc_branch(name, 'add', params.get('add'), C), _gc_branch(name, 'mul', params.get('mul'), C)
    _gc_planes(name, add, mul)
    if identity is not None:
        if tuple(identity.shape) != tuple(x.shape):
            raise ValueError('%s: identity is %s, x %s' % (name, tuple(identity.shape), tuple(x.shape)))
        _gc_vec(name, 'identity', identity, x.numel())
    eps = float(params.get('eps', GC_EPS))
    flat = (w_mask, b_mask) + tuple(params.get('add') or (None,) * 6) + tuple(params.get('mul') or (None,) * 6)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, identity) + flat):
        return _ContextBlockFn.apply(x, identity, bool(relu), eps, *flat)
    return _gc_forward(_c16(x), None if w_mask is None else _c16(w_mask), None if b_mask is None else _c16(b_mask),
                       add[0], mul[0], None if identity is None else _c16(identity), bool(relu), eps)[0]


# ----------------------------------------------------------------------------------------
# sigmoid focal loss  (mmdet/ops/sigmoid_focal_loss, mmdet/models/losses/focal_loss.py)
# ----------------------------------------------------------------------------------------
def _focal_inputs(name, logits, labels, gamma, pos_shift):
    """Checked (float32 logits with unit column stride, row stride, contiguous int64 labels)."""
    if logits.dim() != 2:
        raise ValueError('%s: logits must be [N, C], got %s' % (name, tuple(logits.shape)))
    if logits.dtype != torch.float32:
        raise NotImplementedError('%s: %s logits have no kernel (float32 does)' % (name, logits.dtype))
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.numel() != logits.shape[0]:
        raise ValueError('%s: labels must be int64 [N]' % name)
    if pos_shift not in (0, 1):
        raise ValueError('%s: pos_shift must be 0 or 1' % name)
    if not float(gamma) >= 0.0:
        raise ValueError('%s: gamma must be >= 0' % name)
    if logits.shape[0] * logits.shape[1] >= 2 ** 31:
        raise NotImplementedError('%s: N * C >= 2^31' % name)
    z = logits.detach()
    if z.shape[0] > 1 and (z.stride(1) != 1 or z.stride(0) < z.shape[1]) or z.shape[0] <= 1 and not z.is_contiguous():
        z = z.contiguous()
    ld = z.stride(0) if z.shape[0] > 1 else z.shape[1]
    return z, int(ld), labels.contiguous()


class _SigmoidFocalLoss(torch.autograd.Function):
    """Reduced loss and dense gradient from ONE launch (``bgs_sigmoid_focal_fwd_bwd``); backward only scales the
    kept ``dlogits`` by the upstream scalar."""

    @staticmethod
    def forward(ctx, logits, labels, row_weights, cls_weight, gamma, alpha, avg, loss_weight, pos_shift):
        lib = capi.load()
        z, ld, labels = _focal_inputs('sigmoid_focal_loss', logits, labels, gamma, pos_shift)
        N, C = z.shape
        dev = z.device
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        dlogits = torch.empty((N, C), dtype=torch.float32, device=dev) if logits.requires_grad else None
        ws = _workspace(lib.bgs_sigmoid_focal_workspace_bytes(), dev)
        rc = lib.bgs_sigmoid_focal_fwd_bwd(capi.ptr(z), ld, capi.ptr(labels), capi.ptr(row_weights),
                                           capi.ptr(cls_weight), N, C, float(gamma), float(alpha), int(pos_shift),
                                           capi.ptr(avg), float(loss_weight), capi.ptr(loss), capi.ptr(dlogits),
                                           capi.ptr(ws), capi.current_stream(dev))
        capi.check('bgs_sigmoid_focal_fwd_bwd', rc)
        ctx.dlogits = dlogits
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        if ctx.dlogits is None:
            return (None,) * 9
        return (ctx.dlogits * grad_loss,) + (None,) * 8


def sigmoid_focal_loss(logits, labels, row_weights=None, cls_weight=None, gamma=2.0, alpha=0.25, avg=None,
                       loss_weight=1.0, pos_shift=0):
    """``loss_weight * sum_r w_r sum_d focal(logits[r, d]) / avg`` as a scalar, differentiable w.r.t. ``logits``.

    ``labels [N] i64``: the positive column of row ``r`` is ``labels[r] - pos_shift`` when that lies in ``[0, C)``,
    otherwise the row has none.  ``w_r = row_weights[r] * cls_weight[labels[r]]`` (either may be ``None`` = 1); the
    gather runs inside the kernel and a label outside ``[0, C)`` gets weight 0.  ``avg``: a number, a device float
    tensor ``[1]`` (no sync), or ``None`` = ``N * C``."""
    _require_cuda(logits, labels, row_weights, cls_weight)
    N, C = logits.shape
    if row_weights is not None:
        row_weights = _f32c(row_weights).reshape(-1)
        if row_weights.numel() != N:
            raise ValueError('sigmoid_focal_loss: row_weights must hold N values')
    if cls_weight is not None:
        cls_weight = _f32c(cls_weight).reshape(-1)
        if cls_weight.numel() != C:
            raise ValueError('sigmoid_focal_loss: cls_weight must hold C values')
    if avg is not None:
        if isinstance(avg, torch.Tensor):
            _require_cuda(avg)
            avg = _f32c(avg).reshape(-1)[:1]
        else:
            avg = torch.full((1,), float(avg), dtype=torch.float32, device=logits.device)
    return _SigmoidFocalLoss.apply(logits, labels, row_weights, cls_weight, gamma, alpha, avg, loss_weight,
                                   pos_shift)


class _SigmoidFocalElementwise(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, labels, gamma, alpha, pos_shift):
        lib = capi.load()
        z, ld, labels = _focal_inputs('sigmoid_focal_loss_elementwise', logits, labels, gamma, pos_shift)
        N, C = z.shape
        losses = torch.empty((N, C), dtype=torch.float32, device=z.device)
        rc = lib.bgs_sigmoid_focal_fwd(capi.ptr(z), ld, capi.ptr(labels), N, C, float(gamma), float(alpha),
                                       int(pos_shift), capi.ptr(losses), capi.current_stream(z.device))
        capi.check('bgs_sigmoid_focal_fwd', rc)
        ctx.save_for_backward(z, labels)
        ctx.cfg = (ld, float(gamma), float(alpha), int(pos_shift))
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_losses):
        z, labels = ctx.saved_tensors
        ld, gamma, alpha, pos_shift = ctx.cfg
        lib = capi.load()
        N, C = z.shape
        d = _f32c(d_losses)
        d_logits = torch.empty((N, C), dtype=torch.float32, device=z.device)
        rc = lib.bgs_sigmoid_focal_bwd(capi.ptr(z), ld, capi.ptr(labels), capi.ptr(d), N, C, gamma, alpha,
                                       pos_shift, capi.ptr(d_logits), capi.current_stream(z.device))
        capi.check('bgs_sigmoid_focal_bwd', rc)
        return d_logits, None, None, None, None


def sigmoid_focal_loss_elementwise(logits, labels, gamma=2.0, alpha=0.25, pos_shift=0):
    """The unreduced ``[N, C]`` focal losses (``bgs_sigmoid_focal_fwd``), differentiable through
    ``bgs_sigmoid_focal_bwd``; label convention of :func:`sigmoid_focal_loss`."""
    _require_cuda(logits, labels)
    return _SigmoidFocalElementwise.apply(logits, labels, gamma, alpha, pos_shift)


def fc_reg_gather_enabled():
    """A frozen class-specific ``fc_reg`` computes only the four columns of each RoI's own class
    (``ConvFCBBoxHead.forward(reg_labels=...)``): ``BGS_FC_REG_GATHER=0`` (read per call) keeps the dense launch."""
    return os.environ.get('BGS_FC_REG_GATHER', '1') != '0'


def fc_reg_gather(x, weight, bias, labels):
    """``y[r, 0:4] = x[r] . weight[4 l : 4 l + 4].T + bias[4 l : 4 l + 4]`` with ``l = labels[r]`` (zeros for a label
    outside ``[0, weight.shape[0] / 4)``): the slot of the dense ``fc_reg`` output that the box loss and
    ``refine_boxes`` read, without the other columns.  No autograd: for a frozen ``fc_reg`` only."""
    _require_cuda(x, weight, bias, labels)
    lib = capi.load()
    assert x.dim() == 2 and weight.dim() == 2 and weight.shape[1] == x.shape[1] and weight.shape[0] % 4 == 0
    assert labels.dtype == torch.int64 and labels.numel() == x.shape[0]
    x, w = _f32c(x), _f32c(weight)
    b = None if bias is None else _f32c(bias)
    K, C = x.shape
    y = torch.empty((K, 4), dtype=torch.float32, device=x.device)
    rc = lib.bgs_fc_reg_gather(capi.ptr(x), capi.ptr(w), capi.ptr(b), capi.ptr(labels.contiguous()), K, C,
                               w.shape[0] // 4, capi.ptr(y), capi.current_stream(x.device))
    capi.check('bgs_fc_reg_gather', rc)
    return y


# ----------------------------------------------------------------------------------------
# conv / linear on the matrix cores (NHWC fp32 activations, [Cout,R,S,Cin] fp32 weights)
#   math 'bf16x6' (default): bf16 MFMA on exactly split operands, fp32-faithful (csrc/conv_bfx.hip)
#   math 'f32':              v_mfma_f32_32x32x2_f32 (csrc/conv_igemm.hip, csrc/conv_halo.hip)
#   math 'bf16':             operands rounded to bf16 for the MFMA, fp32 accumulate / storage: the
#                            arithmetic of the reference's fp16 autocast (mmdet/core/fp16/) — cfg[4]
# ----------------------------------------------------------------------------------------
_CONV_MATHS = ('bf16x6', 'f32', 'bf16')


def _checked_conv_math(mode, origin):
    if mode not in _CONV_MATHS:
        raise ValueError('%s: unknown conv math %r (expected one of %s)' % (origin, mode, _CONV_MATHS))
    return mode


# a typo in the environment ('fp32', 'BF16X6') must not select an arithmetic silently: validated at import
_CONV_MATH = [_checked_conv_math(os.environ.get('BGS_CONV_MATH', 'bf16x6'), 'BGS_CONV_MATH')]


def set_conv_math(mode):
    """'bf16x6' | 'f32' | 'bf16'; returns the previous mode.  The first two give fp32-accurate
    results (the split kernel's error against fp64 is not above the fp32 MFMA kernel's; 'f32'
    keeps the bit-exact fp32 fma chain); 'bf16' is the reduced-precision mode of cfg[4]."""
    _checked_conv_math(mode, 'set_conv_math')
    prev = _CONV_MATH[0]
    _CONV_MATH[0] = mode
    return prev


def conv_math():
    return _CONV_MATH[0]


class conv_math_scope(object):
    """``with conv_math_scope('bf16'): ...`` — the mode is restored on exit (also on error)."""

    def __init__(self, mode):
        self.mode = _checked_conv_math(mode, 'conv_math_scope')

    def __enter__(self):
        self.prev = set_conv_math(self.mode)
        return self

    def __exit__(self, *exc):
        set_conv_math(self.prev)
        return False


# Split planes of FROZEN filters only, one entry per storage address: {data_ptr: (version, shape,
# source tensor, planes)}.  The source is kept alive so that its address cannot be handed to another
# tensor while the entry exists; an entry whose version went stale is overwritten in place, so the
# cache never holds more than one split per live frozen tensor.  Trained filters (and per-step
# temporaries such as the folded copies of a trained trunk) are NEVER cached: their split launch is
# part of every step — inside a captured hipGraph it is re-run by every replay, so an eager forward
# after replayed optimizer steps (which do not bump ``_version``) cannot read stale planes.
# bf16 STORAGE of the frozen trunk's activations in the 'bf16' arithmetic mode (csrc/conv_bf16s.hip;
# the memory side of the reference's wrap_fp16_model, mmdet/core/fp16/decorators.py:8-80).
# BGS_BF16_STORAGE=0 keeps fp32 tensors in HBM (operands rounded inside the kernels), the A/B arm.
_BF16_STORAGE = [os.environ.get('BGS_BF16_STORAGE', '1') != '0']


def set_bf16_storage(on):
    """-> previous value.  Effective only while the arithmetic mode is ``'bf16'``."""
    prev = _BF16_STORAGE[0]
    _BF16_STORAGE[0] = bool(on)
    return prev


def bf16_storage_active():
    return _CONV_MATH[0] == 'bf16' and _BF16_STORAGE[0]


# Residual-fork fusion on the trainable trunk (backbone.Bottleneck.run): the block output's ReLU backward and
# the fork's gradient sum ride in the dgrad epilogue of the next block's first conv.  BGS_FORK_FUSION=0: the
# separate threshold / add passes (A/B).
_FORK_FUSION = [os.environ.get('BGS_FORK_FUSION', '1') != '0']


def fork_fusion_enabled():
    return _FORK_FUSION[0]


def set_fork_fusion(on):
    prev = _FORK_FUSION[0]
    _FORK_FUSION[0] = bool(on)
    return prev


_SPLIT_CACHE = {}
_SPLIT_CACHE_MAX = 1024


class CacheFence(object):
    """Orders the FIRST cross-stream use of a cached tensor behind the launches that wrote it (split planes
    and folded weights first built inside a pipeline piece are written on that piece's side stream and then read from
    other streams with nothing in between).  ``CacheFence()`` right after the producing launches records an event on
    the current stream; ``wait()`` before a use makes the current stream wait for it when it is another stream and
    the event has not completed — and forgets the event once it has, so a warm cache costs one attribute test.  Under
    stream capture it does nothing (a captured step is ordered by its own fork / join edges)."""
    __slots__ = ('event', 'stream')

    def __init__(self, device=None):
        self.event = None
        self.stream = None
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            st = torch.cuda.current_stream(device)
            self.event = torch.cuda.Event()
            self.event.record(st)
            self.stream = st.cuda_stream

    def wait(self, device=None):
        ev = self.event
        if ev is None:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        if ev.query():
            self.event = None
            return
        st = torch.cuda.current_stream(device)
        if st.cuda_stream != self.stream:
            st.wait_event(ev)


def clear_split_cache():
    _SPLIT_CACHE.clear()


def bfx_split_weights(w2d, cache=True):
    """``w2d [rows, K]`` fp32 -> the three bf16 planes ``bgs_conv2d_nhwc_f32_bfx_ws`` streams.
    ``cache=True`` declares the tensor FROZEN (the caller decides: a detached view of a trained
    parameter has ``requires_grad == False`` too)."""
    _require_cuda(w2d)
    lib = capi.load()
    assert w2d.dtype == torch.float32 and w2d.dim() == 2 and w2d.is_contiguous()
    rows, K = w2d.shape
    cacheable = cache and not w2d.requires_grad
    key = w2d.data_ptr()
    if cacheable:
        hit = _SPLIT_CACHE.get(key)
        if hit is not None and hit[0] == w2d._version and hit[1] == (rows, K):
            hit[4].wait(w2d.device)
            return hit[3]
    out = torch.empty(lib.bgs_conv_bfx_weight_bytes(rows, K), dtype=torch.uint8, device=w2d.device)
    rc = lib.bgs_conv_bfx_split_weights(capi.ptr(w2d), capi.ptr(out), rows, K,
                                        capi.current_stream(w2d.device))
    capi.check('bgs_conv_bfx_split_weights', rc)
    if cacheable:
        if key not in _SPLIT_CACHE and len(_SPLIT_CACHE) >= _SPLIT_CACHE_MAX:
            _SPLIT_CACHE.pop(next(iter(_SPLIT_CACHE)))      # oldest entry (insertion order)
        _SPLIT_CACHE[key] = (w2d._version, (rows, K), w2d, out, CacheFence(w2d.device))
    return out


def presplit(*weights):
    """Fill the split cache for frozen conv filters ``[Cout,R,S,Cin]`` on the CURRENT stream — before a
    :class:`forked` block whose launches (on two streams) share them."""
    for w in weights:
        if w is not None and w.is_cuda and w.dim() == 4 and not w.requires_grad and \
                (_CONV_MATH[0] != 'f32' or bf16_storage_active()):
            bfx_split_weights(w.view(w.shape[0], -1), cache=True)


def bfx_split_weights_dgrad(w_krsc, cache=True):
    """The split planes of the DATA-GRADIENT filter of ``w_krsc [Cout,R,S,Cin]`` (= ``bfx_split_weights``
    of ``dgrad_filter(w_krsc).view(Cin, R*S*Cout)``) in one launch (``bgs_conv_bfx_split_weights_dgrad``).
    ``cache`` as in :func:`bfx_split_weights`."""
    _require_cuda(w_krsc)
    lib = capi.load()
    assert w_krsc.dtype == torch.float32 and w_krsc.dim() == 4 and w_krsc.is_contiguous()
    Cout, R, S, Cin = w_krsc.shape
    cacheable = cache and not w_krsc.requires_grad
    key = (w_krsc.data_ptr(), 'dgrad')
    if cacheable:
        hit = _SPLIT_CACHE.get(key)
        if hit is not None and hit[0] == w_krsc._version and hit[1] == (Cout, R, S, Cin):
            hit[4].wait(w_krsc.device)
            return hit[3]
    out = torch.empty(lib.bgs_conv_bfx_weight_bytes(Cin, R * S * Cout), dtype=torch.uint8,
                      device=w_krsc.device)
    rc = lib.bgs_conv_bfx_split_weights_dgrad(capi.ptr(w_krsc), capi.ptr(out), Cout, R, S, Cin,
                                              capi.current_stream(w_krsc.device))
    capi.check('bgs_conv_bfx_split_weights_dgrad', rc)
    if cacheable:
        if key not in _SPLIT_CACHE and len(_SPLIT_CACHE) >= _SPLIT_CACHE_MAX:
            _SPLIT_CACHE.pop(next(iter(_SPLIT_CACHE)))
        _SPLIT_CACHE[key] = (w_krsc._version, (Cout, R, S, Cin), w_krsc, out, CacheFence(w_krsc.device))
    return out


def conv_bfx_tuning(tile=0, splitk=-1, halo_splits=-1, halo_variant=0, halo_geom=-1, halo_flags=0, halo_wide=-1):
    """Process-wide tuning / test hook of the bf16x6 kernels (see include/bgs_tuning.h).  ``halo_geom``: the
    pixel tile of the halo kernel, -1 default | 0: 8 x 16 | 1: 10 x 12 | 2: 5 x 21 | 3: fewest tiles per image.
    ``halo_wide``: the 16 x 16-pixel units of variant 7, -1 leave as is (the all-default call restores the
    environment's default) | 0 off | 1 automatic | 2 every eligible layer."""
    lib = capi.load()
    lib.bgs_conv_bfx_tuning(int(tile), int(splitk))
    lib.bgs_conv3x3_halo_bfx_tuning(int(halo_splits), int(halo_variant) | ((int(halo_geom) + 1) << 16) |
                                    (int(halo_flags) << 20) | ((int(halo_wide) + 1) << 24))


def set_halo_wide(mode):
    """The wide-pixel-tile mode of the halo 3x3 kernel alone (``bgs_conv3x3_halo_bfx_wide``): -1 environment default |
    0 off | 1 automatic schedule | 2 every eligible layer; returns the previous mode."""
    return capi.load().bgs_conv3x3_halo_bfx_wide(int(mode))


def conv_bfx_last_launch():
    """-> dict(tile, splits, halo_nb, halo_splits, ...) of the last bf16x6 launches.  ``halo_variant`` 7: the wide
    pixel tile ran (``halo_wide_units`` 256-pixel units) followed by ``halo_tail_units`` 128-pixel units on variant 4."""
    import ctypes
    lib = capi.load()
    a, c, d, e, f, g = (ctypes.c_int() for _ in range(6))
    lib.bgs_conv_bfx_last_launch(ctypes.byref(a), ctypes.byref(c))
    lib.bgs_conv3x3_halo_bfx_last_launch(ctypes.byref(d), ctypes.byref(e))
    lib.bgs_conv3x3_halo_bfx_last_wide(ctypes.byref(f), ctypes.byref(g))
    return dict(tile=a.value & ~0x400, ring_stages=3 if a.value & 0x400 else 4, splits=c.value,
                halo_nb=d.value & 0xff, halo_variant=(d.value >> 8) & 0xff, halo_geom=d.value >> 16,
                halo_splits=e.value, halo_wide_units=f.value, halo_tail_units=g.value)


CENSUS = dict(bf16_ring8=0, grouped_lds=1, halo_bfx4=2, dma_ring64=3, gs_head_fused=4, conv1x1_bres=5,
              wgrad_bfx=6, roi_bwd_gather=7, bf16s=8, grouped_bf16s=9, bfx_wide=10, gs_scale_grad=11, halo_wide=12, stem_fused=13, fused_c3=14,
              planes_3x3=15, planes_1x1=16, planes_3x3_head=17, fused_c3_next=18, fused_c3_shortcut=19)


def launch_census(reset=False):
    """-> {family: launches since the last reset} (``bgs_launch_census``; include/bgs.h BGS_CENSUS_*)."""
    lib = capi.load()
    out = {k: lib.bgs_launch_census(v, 0) for k, v in CENSUS.items()}
    if reset:
        lib.bgs_launch_census(0, 1)
    return out


def conv_tuning(tile=0, bk=0, splitk=0, noswizzle=0):
    """Process-wide tuning / test hook of the fp32 MFMA conv kernel (see include/bgs.h)."""
    capi.load().bgs_conv_tuning(int(tile), int(bk), int(splitk), int(noswizzle))


def conv_last_launch():
    """-> dict(tile, bk, up, splits) of the last fp32 MFMA conv launch."""
    import ctypes
    a, b, c, d = (ctypes.c_int() for _ in range(4))
    capi.load().bgs_conv_last_launch(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
    return dict(tile=a.value, bk=b.value, up=c.value, splits=d.value)


def _use_halo_bfx(M, Cout):
    """bf16x6 path: the halo kernel wins on every 3x3 stride-1 layer of cfg[1] down to the 25x42
    maps (profiles/r2g_bfx_sweep.txt: P2 0.74 vs 1.01 ms, P3 0.22 vs 0.28, M = 8400: 0.078 vs
    0.089, M = 2100: 0.035 vs 0.039); the 13x21 level (M = 546) stays on the general kernel."""
    env = os.environ.get('BGS_CONV_HALO')
    if env == '1':
        return True
    if env == '0':
        return False
    return M >= 2000


def _use_halo_kernel(M, Cout):
    """``BGS_CONV_HALO`` = 1: every eligible 3x3 layer, 0: never; unset: where it was measured
    faster than the general kernel (tools/conv_halo_check.py, profiles/r3m_conv_halo.txt): the
    large-M, Cout % 128 == 0 layers (FPN output conv and RPN conv on P2: 114 vs 98 TFLOP/s); its
    fixed 128 x 128 tile without split-K loses on the smaller ones."""
    env = os.environ.get('BGS_CONV_HALO')
    if env == '1':
        return True
    if env == '0':
        return False
    return M >= 100000 and Cout % 128 == 0


_FUSED_C3 = [os.environ.get('BGS_FUSED_C3', '1') != '0']


def set_fused_c3(on):
    """-> previous value.  ``BGS_FUSED_C3=0`` / ``set_fused_c3(False)``: a frozen bottleneck runs conv2 and conv3 as two
    launches (the A/B arm; bit-identical)."""
    prev = _FUSED_C3[0]
    _FUSED_C3[0] = bool(on)
    return prev


def fused_c3_eligible(x, w2, w3, stride, residual):
    """conv2 -> conv3 of a frozen bottleneck in one launch (``bgs_conv3x3_c3_fused_nhwc_f32_bfx``, round 6): fp32 NHWC
    activations under the fp32-faithful arithmetic, 3x3 / stride 1, 64 -> 64 -> 256 channels (ResNet-50 layer1), the map
    large enough for the halo kernel and within the fused kernel's size bound (``bgs_conv3x3_c3_fused_eligible``; a
    larger map runs the two launches), nothing that needs a gradient."""
    env = os.environ.get('BGS_FUSED_C3')              # (read at every call: tools/step_ab.py switches it between arms)
    on = _FUSED_C3[0] if env is None else env != '0'
    return (on and _CONV_MATH[0] == 'bf16x6' and x.is_cuda and x.dtype == torch.float32 and stride == 1
            and tuple(w2.shape[:3]) == (64, 3, 3) and w2.shape[3] == 64 and tuple(w3.shape) == (256, 1, 1, 64)
            and x.shape[3] == 64 and _use_halo_bfx(x.shape[0] * x.shape[1] * x.shape[2], 64)
            # (>= 700 pixel tiles: below that the unfused conv2 splits its channel chunks over gridDim.z — another
            #  summation order — and a short grid gains nothing from the fusion; csrc/conv3x3_halo_bfx.hip halo_bfx_plan)
            and x.shape[0] * ((x.shape[1] + 7) // 8) * ((x.shape[2] + 15) // 16) >= 700
            and not (torch.is_grad_enabled() and (x.requires_grad or w2.requires_grad or w3.requires_grad or
                                                  (residual is not None and residual.requires_grad)))
            and bool(capi.load().bgs_conv3x3_c3_fused_eligible(x.shape[0], x.shape[1], x.shape[2], 64, 256)))


def _c3_tail(x, w2_krsc, bias2, w3_krsc, bias3, residual=None, relu3=True, out=None, w1n_krsc=None, bias1n=None,
             x0=None, w_sc_krsc=None, bias_sc=None):
    """The one body of the three tail wrappers below -> ``(y, h)``: the checks, the filter splits, the allocations and
    the choice of entry point.  ``x0`` given: the projection-shortcut form (no ``residual``); ``w1n_krsc`` given: ``h``,
    the next block's conv1 (else ``h`` is None)."""
    _require_cuda(x, w2_krsc, bias2, w3_krsc, bias3, residual, w1n_krsc, bias1n, x0, w_sc_krsc, bias_sc)
    lib = capi.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    N, H, W, Cmid = x.shape
    Cout3 = w3_krsc.shape[0]
    Cnext = 0 if w1n_krsc is None else w1n_krsc.shape[0]
    assert tuple(w2_krsc.shape) == (Cmid, 3, 3, Cmid) and tuple(w3_krsc.shape) == (Cout3, 1, 1, Cmid)
    if residual is not None:
        assert tuple(residual.shape) == (N, H, W, Cout3) and residual.is_contiguous() and residual.dtype == torch.float32
    y = out if out is not None else torch.empty((N, H, W, Cout3), dtype=torch.float32, device=x.device)
    w2s = bfx_split_weights(w2_krsc.view(Cmid, 9 * Cmid), cache=True)
    w3s = bfx_split_weights(w3_krsc.view(Cout3, Cmid), cache=True)
    h = w1s = None
    if Cnext:
        assert tuple(w1n_krsc.shape) == (Cnext, 1, 1, Cout3) and w1n_krsc.is_contiguous()
        h = torch.empty((N, H, W, Cnext), dtype=torch.float32, device=x.device)
        w1s = bfx_split_weights(w1n_krsc.view(Cnext, Cout3), cache=True)
    relu3 = int(bool(relu3))
    if x0 is not None:
        Cin0 = x0.shape[3]
        assert residual is None
        assert tuple(x0.shape) == (N, H, W, Cin0) and x0.is_contiguous() and x0.dtype == torch.float32
        assert tuple(w_sc_krsc.shape) == (Cout3, 1, 1, Cin0) and w_sc_krsc.is_contiguous()
        wss = bfx_split_weights(w_sc_krsc.view(Cout3, Cin0), cache=True)
        name = 'bgs_conv3x3_c3_sc_fused_nhwc_f32_bfx'
        tensors = (x, w2s, bias2, w3s, bias3, x0, wss, bias_sc, y, w1s, bias1n if Cnext else None, h)
        ints = (N, H, W, Cin0, Cmid, Cout3, relu3, Cnext)
    elif Cnext:
        name = 'bgs_conv3x3_c3_next_fused_nhwc_f32_bfx'
        tensors = (x, w2s, bias2, w3s, bias3, residual, y, w1s, bias1n, h)
        ints = (N, H, W, Cmid, Cout3, relu3, Cnext)
    else:
        name = 'bgs_conv3x3_c3_fused_nhwc_f32_bfx'
        tensors = (x, w2s, bias2, w3s, bias3, residual, y)
        ints = (N, H, W, Cmid, Cout3, relu3)
    rc = getattr(lib, name)(*[capi.ptr(t) for t in tensors], *ints, capi.current_stream(x.device))
    capi.check(name, rc)
    return y, h


def conv3x3_c3_fused_nhwc(x, w2_krsc, bias2, w3_krsc, bias3, residual=None, relu3=True, out=None):
    """``y = act(conv1x1(relu(conv3x3(x, w2) + bias2), w3) + bias3 + residual)`` in ONE launch (the second half of a frozen
    bottleneck, resnet.py:239-266); bit-identical to the two ``conv2d_nhwc`` calls it replaces."""
    return _c3_tail(x, w2_krsc, bias2, w3_krsc, bias3, residual, relu3, out)[0]


def fused_c3_next_eligible(x, w2, w3, stride, residual, w1n, b1n=None, stride1n=1, pad1n=0):
    """May the tail of a frozen bottleneck ALSO emit the next block's conv1 (:func:`conv3x3_c3_next_fused_nhwc`)?
    :func:`fused_c3_eligible`, and: that conv1 is 1x1 / stride 1 / no padding with 256 -> 64 or 128 channels, it is frozen
    and nothing needs a gradient, the arithmetic is ``bf16x6`` on fp32 storage.  ``BGS_TAIL_NEXT_C1=0`` (read per call):
    the launches of before."""
    if os.environ.get('BGS_TAIL_NEXT_C1', '1') == '0':
        return False
    if w1n is None or w1n.dim() != 4 or stride1n != 1 or pad1n != 0:
        return False
    if tuple(w1n.shape[1:]) != (1, 1, 256) or w1n.shape[0] not in (64, 128) or w1n.dtype != torch.float32:
        return False
    if torch.is_grad_enabled() and (w1n.requires_grad or (b1n is not None and b1n.requires_grad)):
        return False
    if not fused_c3_eligible(x, w2, w3, stride, residual):
        return False
    N, H, W, _ = x.shape
    return bool(capi.load().bgs_conv3x3_c3_next_eligible(N, H, W, 64, 256, w1n.shape[0]))


def conv3x3_c3_next_fused_nhwc(x, w2_krsc, bias2, w3_krsc, bias3, w1n_krsc, bias1n, residual=None, relu3=True):
    """:func:`conv3x3_c3_fused_nhwc` with the NEXT block's conv1 in the same launch -> ``(y, h)``,
    ``h = relu(conv1x1(y, w1n) + bias1n)`` ``[N,H,W,Cnext]``; both bit-identical to the two calls it replaces
    (``conv3x3_c3_fused_nhwc``, then ``conv2d_nhwc(y, w1n, bias1n, relu=True)``).  Forward only, frozen filters."""
    return _c3_tail(x, w2_krsc, bias2, w3_krsc, bias3, residual, relu3, w1n_krsc=w1n_krsc, bias1n=bias1n)


def fused_c3_shortcut_eligible(x0, h1_shape, w2, w3, stride, w_sc, b_sc=None, stride_sc=1):
    """May the tail of a frozen bottleneck compute the block's own projection shortcut (:func:`conv3x3_c3_sc_fused_nhwc`)
    in place of reading the map a shortcut launch wrote?  ``x0``: the block input, ``h1_shape``: the shape of conv1's
    output (the tail's input; conv1 is 1x1 / stride 1, so it is known from ``x0``).  :func:`fused_c3_eligible` on that
    shape, and: the shortcut is 1x1 / stride 1 with 64 -> 256 channels, it is frozen and nothing needs a gradient, the
    arithmetic is ``bf16x6`` on fp32 storage.  ``BGS_TAIL_SHORTCUT=0`` (read per call): the launches of before."""
    if os.environ.get('BGS_TAIL_SHORTCUT', '1') == '0':
        return False
    if w_sc is None or w_sc.dim() != 4 or stride_sc != 1 or stride != 1:
        return False
    if tuple(w_sc.shape) != (256, 1, 1, 64) or w_sc.dtype != torch.float32 or not w_sc.is_contiguous():
        return False
    if x0.dim() != 4 or x0.shape[3] != 64 or x0.dtype != torch.float32 or not x0.is_cuda or not x0.is_contiguous():
        return False
    if tuple(h1_shape) != (x0.shape[0], x0.shape[1], x0.shape[2], 64):
        return False
    if torch.is_grad_enabled() and (x0.requires_grad or w_sc.requires_grad or (b_sc is not None and b_sc.requires_grad)):
        return False
    # (the tail's own rule; x0 stands in for conv1's output: same device, dtype and shape, and neither needs a gradient)
    if not fused_c3_eligible(x0, w2, w3, stride, None):
        return False
    N, H, W, _ = x0.shape
    return bool(capi.load().bgs_conv3x3_c3_sc_eligible(N, H, W, 64, 64, 256, 0))


def conv3x3_c3_sc_fused_nhwc(x, w2_krsc, bias2, w3_krsc, bias3, x0, w_sc_krsc, bias_sc, w1n_krsc=None, bias1n=None,
                             relu3=True):
    """:func:`conv3x3_c3_fused_nhwc` with ``residual = conv1x1(x0, w_sc) + bias_sc`` — the block's 1x1 / stride-1
    projection shortcut on the block input ``x0`` ``[N,H,W,64]`` — computed inside the launch -> ``y``; with ``w1n_krsc``
    (the next block's conv1, 256 -> 64) -> ``(y, h)`` as :func:`conv3x3_c3_next_fused_nhwc`.  Bit-identical to
    ``conv2d_nhwc(x0, w_sc, bias_sc)`` followed by those calls.  Forward only, frozen filters."""
    y, h = _c3_tail(x, w2_krsc, bias2, w3_krsc, bias3, None, relu3, w1n_krsc=w1n_krsc, bias1n=bias1n, x0=x0,
                    w_sc_krsc=w_sc_krsc, bias_sc=bias_sc)
    return y if h is None else (y, h)


def rpn_head_fusion_eligible(x, w_conv, w_head):
    """May ``conv1x1(relu(conv3x3(x, w_conv)), w_head)`` run as ONE launch (:func:`conv3x3_head_fused_nhwc`) in place of
    the two it is bit-identical to?  Nothing may need a gradient (the 256-channel map is never stored), the arithmetic is
    ``bf16x6`` on fp32 activations, and the default dispatch puts this map on the 256-channel 3x3 planes kernel with the
    head unsliced (``bgs_conv3x3_planes_head_eligible``).  ``BGS_RPN_HEAD_FUSION=0`` (read per call): the two launches."""
    if os.environ.get('BGS_RPN_HEAD_FUSION', '1') == '0' or _CONV_MATH[0] != 'bf16x6':
        return False
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or w_conv.dim() != 4 or w_head.dim() != 4:
        return False
    N, H, W, Cin = x.shape
    if tuple(w_conv.shape[1:]) != (3, 3, Cin) or tuple(w_head.shape[1:]) != (1, 1, w_conv.shape[0]):
        return False
    if not _use_halo_bfx(N * H * W, w_conv.shape[0]):
        return False
    return bool(capi.load().bgs_conv3x3_planes_head_eligible(N, H, W, Cin, w_conv.shape[0], w_head.shape[0]))


def conv3x3_head_fused_nhwc(x, w_krsc, bias, hw_krsc, hbias, relu=True):
    """``y [N,H,W,Chead] = conv1x1(act(conv3x3(x, w) + bias), hw) + hbias`` in ONE launch
    (``bgs_conv3x3_planes_head_nhwc_f32_bfx``: ``rpn_conv`` with ``rpn_cls + rpn_reg`` in its epilogue); bit-identical to
    the two ``conv2d_nhwc`` calls on the maps :func:`rpn_head_fusion_eligible` accepts.  Forward only, frozen filters."""
    _require_cuda(x, w_krsc, bias, hw_krsc, hbias)
    lib = capi.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    N, H, W, Cin = x.shape
    Cout, Ch = w_krsc.shape[0], hw_krsc.shape[0]
    assert tuple(w_krsc.shape) == (Cout, 3, 3, Cin) and tuple(hw_krsc.shape) == (Ch, 1, 1, Cout)
    assert w_krsc.is_contiguous() and hw_krsc.is_contiguous()
    ws = bfx_split_weights(w_krsc.view(Cout, 9 * Cin), cache=True)
    hs = bfx_split_weights(hw_krsc.view(Ch, Cout), cache=True)
    out = torch.empty((N, H, W, Ch), dtype=torch.float32, device=x.device)
    rc = lib.bgs_conv3x3_planes_head_nhwc_f32_bfx(capi.ptr(x), capi.ptr(ws), capi.ptr(bias), capi.ptr(hs),
                                                  capi.ptr(hbias), capi.ptr(out), N, H, W, Cin, Cout,
                                                  int(bool(relu)), Ch, capi.current_stream(x.device))
    capi.check('bgs_conv3x3_planes_head_nhwc_f32_bfx', rc)
    return out


def conv2d_nhwc(x, w_krsc, bias=None, stride=1, pad=0, relu=False, residual=None,
                residual_mode=0, out=None, frozen_weight=True, out_dtype=None):
    """``y = act(conv(x, w) + bias + residual)``; x ``[N,H,W,Cin]``, w ``[Cout,R,S,Cin]``.
    Forward only (the shipped BAGS configs freeze every conv: selectp=1, tools/train.py:49-57).
    ``frozen_weight=False``: ``w_krsc`` is (a detached view of) a tensor that changes from step to
    step — its bf16 planes are split on every call and never cached.
    ``x`` in bf16 selects the bf16 storage kernels (cfg[4] bf16 mode; ``out_dtype``: bf16 (default)
    or fp32 for consumers outside the trunk)."""
    _require_cuda(x, w_krsc, bias, residual)
    lib = capi.load()
    assert x.dtype in (torch.float32, torch.bfloat16) and w_krsc.dtype == torch.float32
    assert x.is_contiguous() and w_krsc.is_contiguous() and x.dim() == 4 and w_krsc.dim() == 4
    N, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w_krsc.shape
    assert Cin == Cin2, (x.shape, w_krsc.shape)
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - S) // stride + 1
    if residual is not None and residual_mode == 0:
        residual_mode = 1
    if residual is not None:
        exp = (N, Ho, Wo, Cout) if residual_mode == 1 else (N, Ho // 2, Wo // 2, Cout)
        assert tuple(residual.shape) == exp and residual.is_contiguous(), (residual.shape, exp)
    if x.dtype == torch.bfloat16:
        # bf16 storage mode (csrc/conv_bf16s.hip): bf16 activations, the bf16(w) plane, fp32 accumulate
        if out_dtype is None:
            out_dtype = torch.bfloat16
        assert out_dtype in (torch.float32, torch.bfloat16)
        assert residual is None or residual.dtype in (torch.float32, torch.bfloat16)
        if out is None:
            out = torch.empty((N, Ho, Wo, Cout), dtype=out_dtype, device=x.device)
        assert out.dtype == out_dtype
        wsplit = bfx_split_weights(w_krsc.view(Cout, R * S * Cin), cache=bool(frozen_weight))
        rc = lib.bgs_conv2d_nhwc_bf16s(capi.ptr(x), capi.ptr(wsplit), capi.ptr(bias), capi.ptr(residual),
                                       residual_mode if residual is not None else 0,
                                       int(residual is not None and residual.dtype == torch.bfloat16),
                                       capi.ptr(out), int(out_dtype == torch.bfloat16), N, H, W, Cin,
                                       Cout, R, S, stride, pad, int(bool(relu)),
                                       capi.current_stream(x.device))
        capi.check('bgs_conv2d_nhwc_bf16s', rc)
        return out
    assert out_dtype in (None, torch.float32), 'fp32 activations produce fp32 (bf16 out needs bf16 in)'
    assert residual is None or residual.dtype == torch.float32
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    halo_ok = R == 3 and S == 3 and stride == 1 and pad == 1 and residual is None and Cin % 16 == 0
    if _CONV_MATH[0] != 'f32':
        planes = 3 if _CONV_MATH[0] == 'bf16x6' else 1
        wsplit = bfx_split_weights(w_krsc.view(Cout, R * S * Cin), cache=bool(frozen_weight))
        st = capi.current_stream(x.device)
        if halo_ok and _use_halo_bfx(N * Ho * Wo, Cout):
            wsb = lib.bgs_conv3x3_halo_bfx_workspace_bytes(N, H, W, Cin, Cout)
            ws = _workspace(wsb, x.device) if wsb else None
            rc = lib.bgs_conv3x3_halo_nhwc_f32_bfx(capi.ptr(x), capi.ptr(wsplit), capi.ptr(bias),
                                                   capi.ptr(out), N, H, W, Cin, Cout,
                                                   int(bool(relu)), planes, capi.ptr(ws), wsb, st)
            capi.check('bgs_conv3x3_halo_nhwc_f32_bfx', rc)
            return out
        wsb = lib.bgs_conv_bfx_workspace_bytes(N * Ho * Wo, Cout, R * S * Cin)
        ws = _workspace(wsb, x.device) if wsb else None
        rc = lib.bgs_conv2d_nhwc_f32_bfx_ws(capi.ptr(x), capi.ptr(wsplit), capi.ptr(bias),
                                            capi.ptr(residual), capi.ptr(out), N, H, W, Cin, Cout,
                                            R, S, stride, pad, int(bool(relu)), residual_mode,
                                            planes, capi.ptr(ws), wsb, st)
        capi.check('bgs_conv2d_nhwc_f32_bfx_ws', rc)
        return out
    if halo_ok and _use_halo_kernel(N * Ho * Wo, Cout):
        # halo-resident 3x3 kernel (csrc/conv_halo.hip): the input patch is staged in LDS once per
        # channel chunk and shared by the nine taps
        rc = lib.bgs_conv3x3_halo_nhwc_f32(capi.ptr(x), capi.ptr(w_krsc), capi.ptr(bias),
                                           capi.ptr(out), N, H, W, Cin, Cout, int(bool(relu)),
                                           capi.current_stream(x.device))
        capi.check('bgs_conv3x3_halo_nhwc_f32', rc)
        return out
    wsb = lib.bgs_conv2d_workspace_bytes(N * Ho * Wo, Cout)      # split-K scratch (small-M layers)
    ws = _workspace(wsb, x.device) if wsb else None
    rc = lib.bgs_conv2d_nhwc_f32_ws(capi.ptr(x), capi.ptr(w_krsc), capi.ptr(bias),
                                    capi.ptr(residual), capi.ptr(out), N, H, W, Cin, Cout, R, S,
                                    stride, pad, int(bool(relu)), residual_mode, capi.ptr(ws),
                                    wsb, capi.current_stream(x.device))
    capi.check('bgs_conv2d_nhwc_f32_ws', rc)
    return out


def dgrad_filter(w_krsc):
    """``[Cout,R,S,Cin]`` -> ``[Cin,R,S,Cout]`` with both spatial axes flipped: the filter layout
    ``bgs_conv2d_dgrad_nhwc_f32`` streams (K-major for the transposed problem)."""
    return w_krsc.detach().permute(3, 1, 2, 0).flip(1, 2).contiguous()


def conv2d_dgrad_nhwc(dy, w_krsc, in_hw, stride=1, pad=0, residual=None, residual_mode=0,
                      mask=None, wt=None, frozen_weight=False):
    """Data gradient of :func:`conv2d_nhwc`: ``dy [N,Ho,Wo,Cout]`` -> ``dx [N,H,W,Cin]``.
    ``residual`` is added (mode 1 same shape, mode 3: ``[N,2H,2W,Cin]`` 2x2-sum-pooled), then
    ``mask > 0`` gates the result (ReLU backward of the conv's input)."""
    _require_cuda(dy, w_krsc, residual, mask)
    lib = capi.load()
    assert dy.dtype == torch.float32 and dy.is_contiguous() and dy.dim() == 4
    Cout, R, S, Cin = w_krsc.shape
    N, Ho, Wo, Cout2 = dy.shape
    H, W = in_hw
    assert Cout == Cout2 and Ho == (H + 2 * pad - R) // stride + 1 and \
        Wo == (W + 2 * pad - S) // stride + 1, (dy.shape, w_krsc.shape, in_hw)
    if Cout % 4 != 0:      # e.g. the fused RPN head (15 outputs): zero-pad the reduction axis
        padc = 4 - Cout % 4
        dy = torch.nn.functional.pad(dy, (0, padc))
        w_krsc = torch.nn.functional.pad(w_krsc.detach(), (0, 0, 0, 0, 0, 0, 0, padc))
        Cout += padc
        wt = None
    wt_is_temp = wt is None
    fused_split = wt is None and _CONV_MATH[0] != 'f32' and os.environ.get('BGS_DGRAD_FUSED_SPLIT', '1') != '0'
    if wt is None and not fused_split:
        wt = dgrad_filter(w_krsc)
    if residual is not None and residual_mode == 0:
        residual_mode = 1
    if residual is not None:
        exp = (N, H, W, Cin) if residual_mode == 1 else (N, 2 * H, 2 * W, Cin)
        assert tuple(residual.shape) == exp and residual.is_contiguous(), (residual.shape, exp)
    if mask is not None:
        assert tuple(mask.shape) == (N, H, W, Cin) and mask.is_contiguous()
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dy.device)
    if _CONV_MATH[0] != 'f32':
        if fused_split:
            # flip + transpose + split in one launch; cached for frozen filters (a detached view of a
            # trained filter changes from step to step: w_krsc.requires_grad tells nothing about it,
            # so only tensors the caller passes as frozen parameters are cached — see _ConvFn.backward)
            wt_split = bfx_split_weights_dgrad(w_krsc.detach().contiguous(), cache=bool(frozen_weight))
        else:
            wt_split = bfx_split_weights(wt.view(Cin, R * S * Cout), cache=not wt_is_temp)
        if R == 3 and S == 3 and stride == 1 and pad == 1 and residual is None and Cout % 16 == 0 \
                and _use_halo_bfx(N * H * W, Cin) and os.environ.get('BGS_DGRAD_HALO', '1') != '0':
            # the data gradient of a 3x3 / stride 1 / pad 1 conv is the same conv of dy with the
            # flipped, transposed filter: the halo-resident kernel of the forward pass (ReLU-backward
            # mask in its epilogue) instead of the general operand ring
            wsb = lib.bgs_conv3x3_halo_bfx_workspace_bytes(N, H, W, Cout, Cin)
            ws = _workspace(wsb, dy.device) if wsb else None
            rc = lib.bgs_conv3x3_halo_nhwc_f32_bfx_ex(
                capi.ptr(dy), capi.ptr(wt_split), None, capi.ptr(mask), capi.ptr(dx), N, H, W, Cout,
                Cin, 0, 3 if _CONV_MATH[0] == 'bf16x6' else 1, capi.ptr(ws), wsb,
                capi.current_stream(dy.device))
            if rc == 0:
                return dx
            if rc != 2:          # BGS_ERR_UNSUPPORTED (an A/B variant without the mask): general path
                capi.check('bgs_conv3x3_halo_nhwc_f32_bfx_ex', rc)
        wsb = lib.bgs_conv_bfx_workspace_bytes(N * H * W, Cin, R * S * Cout)
        ws = _workspace(wsb, dy.device) if wsb else None
        rc = lib.bgs_conv2d_dgrad_nhwc_f32_bfx_ws(capi.ptr(dy), capi.ptr(wt_split),
                                                  capi.ptr(residual), capi.ptr(mask), capi.ptr(dx),
                                                  N, H, W, Cin, Cout, R, S, stride, pad,
                                                  residual_mode,
                                                  3 if _CONV_MATH[0] == 'bf16x6' else 1,
                                                  capi.ptr(ws), wsb,
                                                  capi.current_stream(dy.device))
        capi.check('bgs_conv2d_dgrad_nhwc_f32_bfx_ws', rc)
        return dx
    wsb = lib.bgs_conv2d_workspace_bytes(N * H * W, Cin)
    ws = _workspace(wsb, dy.device) if wsb else None
    rc = lib.bgs_conv2d_dgrad_nhwc_f32_ws(capi.ptr(dy), capi.ptr(wt), capi.ptr(residual),
                                          capi.ptr(mask), capi.ptr(dx), N, H, W, Cin, Cout, R, S,
                                          stride, pad, residual_mode, capi.ptr(ws), wsb,
                                          capi.current_stream(dy.device))
    capi.check('bgs_conv2d_dgrad_nhwc_f32_ws', rc)
    return dx


def conv2d_wgrad_nhwc(x, dy, ksize, stride=1, pad=0, bias=False, dw=None, db=None,
                      accumulate=False):
    """Weight (and bias) gradient of :func:`conv2d_nhwc`: ``x [N,H,W,Cin]``, ``dy [N,Ho,Wo,Cout]``
    -> ``dw [Cout,R,S,Cin]`` (``db [Cout]``).  ``accumulate`` adds into the given ``dw``/``db``."""
    _require_cuda(x, dy)
    lib = capi.load()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32
    assert x.is_contiguous() and dy.is_contiguous() and x.dim() == 4 and dy.dim() == 4
    N, H, W, Cin = x.shape
    R = S = int(ksize)
    Cout = dy.shape[3]
    assert tuple(dy.shape[:3]) == (N, (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1)
    dev = x.device
    if Cout % 4 != 0:      # pad the output-channel axis, slice the result
        assert dw is None and db is None and not accumulate
        padc = 4 - Cout % 4
        res = conv2d_wgrad_nhwc(x, torch.nn.functional.pad(dy, (0, padc)), ksize, stride, pad, bias)
        if bias:
            return res[0][:Cout].contiguous(), res[1][:Cout].contiguous()
        return res[:Cout].contiguous()
    if dw is None:
        assert not accumulate
        dw = torch.empty((Cout, R, S, Cin), dtype=torch.float32, device=dev)
    if bias and db is None:
        assert not accumulate
        db = torch.empty((Cout,), dtype=torch.float32, device=dev)
    if _CONV_MATH[0] != 'f32':      # bf16 matrix cores: bf16x6 (fp32-faithful) or bf16 operands
        ws = _workspace(lib.bgs_conv2d_wgrad_bfx_workspace_bytes(N, H, W, Cin, Cout, R, S, stride, pad), dev)
        rc = lib.bgs_conv2d_wgrad_nhwc_f32_bfx(capi.ptr(x), capi.ptr(dy), capi.ptr(dw),
                                               capi.ptr(db) if bias else None, N, H, W, Cin, Cout, R,
                                               S, stride, pad, int(bool(accumulate)),
                                               3 if _CONV_MATH[0] == 'bf16x6' else 1, capi.ptr(ws),
                                               capi.current_stream(dev))
        capi.check('bgs_conv2d_wgrad_nhwc_f32_bfx', rc)
        return (dw, db) if bias else dw
    ws = _workspace(lib.bgs_conv2d_wgrad_workspace_bytes(N, H, W, Cin, Cout, R, S, stride, pad), dev)
    rc = lib.bgs_conv2d_wgrad_nhwc_f32(capi.ptr(x), capi.ptr(dy), capi.ptr(dw),
                                       capi.ptr(db) if bias else None, N, H, W, Cin, Cout, R, S,
                                       stride, pad, int(bool(accumulate)), capi.ptr(ws),
                                       capi.current_stream(dev))
    capi.check('bgs_conv2d_wgrad_nhwc_f32', rc)
    return (dw, db) if bias else dw


class _FoldConvBNFn(torch.autograd.Function):
    """``(w [Cout,Cin,R,S], conv_bias, gamma, beta) -> (wf [Cout,R,S,CinP], bf [Cout])``: eval-mode
    BatchNorm folded into the filter (``bgs_fold_conv_bn_fwd``) with the fold's backward as ONE launch
    (``bgs_fold_conv_bn_bwd``: dw, dconv_bias, dgamma, dbeta) — as tensor ops the fold is ~20
    elementwise / permute launches per conv and step on the `selectp = 0` path."""

    @staticmethod
    def forward(ctx, w, conv_bias, gamma, beta, mean, var, eps, cin_padded):
        lib = capi.load()
        wc = _f32c(w)
        Cout, Cin, R, S = wc.shape
        cinp = int(cin_padded) if cin_padded else Cin
        dev = wc.device
        cb = None if conv_bias is None else _f32c(conv_bias)
        bn = gamma is not None
        g, b_, m, v = (_f32c(t) for t in (gamma, beta, mean, var)) if bn else (None,) * 4
        wf = torch.empty((Cout, R, S, cinp), dtype=torch.float32, device=dev)
        bf = torch.empty((Cout,), dtype=torch.float32, device=dev)
        rc = lib.bgs_fold_conv_bn_fwd(capi.ptr(wc), capi.ptr(cb), capi.ptr(g), capi.ptr(b_),
                                      capi.ptr(m), capi.ptr(v), float(eps), Cout, Cin, R, S, cinp,
                                      capi.ptr(wf), capi.ptr(bf), capi.current_stream(dev))
        capi.check('bgs_fold_conv_bn_fwd', rc)
        ctx.save_for_backward(wc, cb, g, m, v)
        ctx.cfg = (float(eps), cinp, conv_bias is not None, bn)
        return wf, bf

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dwf, dbf):
        wc, cb, g, m, v = ctx.saved_tensors
        eps, cinp, has_cb, bn = ctx.cfg
        lib = capi.load()
        Cout, Cin, R, S = wc.shape
        dev = wc.device
        need = ctx.needs_input_grad
        dw = torch.empty_like(wc) if need[0] else None
        dcb = torch.empty((Cout,), dtype=torch.float32, device=dev) if (has_cb and need[1]) else None
        dg = torch.empty((Cout,), dtype=torch.float32, device=dev) if (bn and need[2]) else None
        db = torch.empty((Cout,), dtype=torch.float32, device=dev) if (bn and need[3]) else None
        rc = lib.bgs_fold_conv_bn_bwd(capi.ptr(dwf.contiguous()), capi.ptr(dbf.contiguous()),
                                      capi.ptr(wc), capi.ptr(cb), capi.ptr(g), capi.ptr(m), capi.ptr(v),
                                      eps, Cout, Cin, R, S, cinp, capi.ptr(dw), capi.ptr(dcb),
                                      capi.ptr(dg), capi.ptr(db), capi.current_stream(dev))
        capi.check('bgs_fold_conv_bn_bwd', rc)
        return dw, dcb, dg, db, None, None, None, None


def fold_conv_bn(weight, conv_bias=None, bn_weight=None, bn_bias=None, running_mean=None,
                 running_var=None, eps=1e-5, cin_padded=None):
    """-> ``(wf [Cout,R,S,CinP], bf [Cout])``, differentiable w.r.t. ``weight``, ``conv_bias``,
    ``bn_weight``, ``bn_bias`` (one launch forward, one backward)."""
    _require_cuda(weight, conv_bias, bn_weight, bn_bias, running_mean, running_var)
    return _FoldConvBNFn.apply(weight, conv_bias, bn_weight, bn_bias, running_mean, running_var,
                               float(eps), cin_padded)


class _ConvFn(torch.autograd.Function):
    """Differentiable fused conv: ``y = act(conv(x, w) + b + residual)`` with gradients for
    x, w, b and the residual (the `selectp = 0` path).

    backward: ``dz = dy * (y > 0)`` (ReLU), ``dx = dgrad(dz, w)``, ``dw, db = wgrad(x, dz)``,
    ``dresidual = dz`` (mode 1) or its 2x2 sum-pool (mode 2: nearest-2x upsampled residual).

    ReLU-backward placement: ``relu='consumers'`` declares that EVERY consumer of ``y`` is a
    ``_ConvFn`` called with ``mask_input=True`` — each of them gates its own ``dx`` with
    ``(y > 0)`` inside the dgrad kernel's epilogue (the mask is linear, so gating the addends
    equals gating their sum) and this node skips the separate masking pass over ``dy``."""

    @staticmethod
    def forward(ctx, x, w, bias, residual, stride, pad, relu, residual_mode, mask_input,
                passthrough=False):
        # w.requires_grad: a trained parameter or the per-step fold of one (its detached view has
        # requires_grad == False, so the decision is taken HERE): split every step, never cached
        y = conv2d_nhwc(x.detach(), w.detach(), None if bias is None else bias.detach(),
                        stride=stride, pad=pad, relu=bool(relu),
                        residual=None if residual is None else residual.detach(),
                        residual_mode=residual_mode, frozen_weight=not w.requires_grad)
        ctx.cfg = (stride, pad, relu, residual_mode if residual is not None else 0,
                   bias is not None, mask_input)
        ctx.math = _CONV_MATH[0]          # backward replays in the arithmetic of this forward
        ctx.save_for_backward(x, w, y if relu is True else None)
        if passthrough:
            # second output: an alias of x for the OTHER consumer of x at a fork (the identity path
            # of a residual block).  Its gradient arrives in this node's backward together with
            # dy, so the fork's `g_conv + g_identity` is the dgrad kernel's residual epilogue
            # instead of a separate pass over the map
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dalias=None):
        x, w, y = ctx.saved_tensors
        stride, pad, relu, res_mode, has_bias, mask_input = ctx.cfg
        if dy is None:            # (passthrough nodes only: y itself had no consumer)
            return (dalias,) + (None,) * 9
        dz = dy.contiguous()
        if relu is True:          # one fused pass: dy * (y > 0)
            dz = torch.ops.aten.threshold_backward(dz, y, 0.0)
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        dx = dw = db = dres = None
        with conv_math_scope(ctx.math):
            if need_x:
                dx = conv2d_dgrad_nhwc(dz, w, (x.shape[1], x.shape[2]), stride=stride, pad=pad,
                                       residual=None if dalias is None else dalias.contiguous(),
                                       mask=x if mask_input else None,
                                       frozen_weight=not w.requires_grad)
            if need_w or (has_bias and need_b):
                out = conv2d_wgrad_nhwc(x, dz, w.shape[1], stride=stride, pad=pad, bias=has_bias)
                dw, db = out if has_bias else (out, None)
        if res_mode and need_r:
            if res_mode == 1:
                dres = dz
            else:
                n, h, wd, c = dz.shape
                dres = dz.view(n, h // 2, 2, wd // 2, 2, c).sum(dim=(2, 4))
        return dx, dw, db, dres, None, None, None, None, None, None


class _ReluGateFn(torch.autograd.Function):
    """Identity whose backward applies the ReLU gate of its (post-ReLU) input: turns a
    ``relu='consumers'`` conv output into an ordinary tensor that ANY consumer may use."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return y.view_as(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return torch.ops.aten.threshold_backward(g.contiguous(), y, 0.0)


def relu_gate(y):
    """Public-boundary adapter for ``relu='consumers'`` outputs (see :class:`_ConvFn`): the
    returned tensor carries the ReLU backward itself.  No-op when nothing is being recorded."""
    if torch.is_grad_enabled() and y.requires_grad and getattr(y, '_bgs_consumers_mask', False):
        return _ReluGateFn.apply(y)
    return y


def conv2d_autograd(x, w_krsc, bias=None, stride=1, pad=0, relu=False, residual=None,
                    residual_mode=0, mask_input=False, out_dtype=None, passthrough=False):
    """:func:`conv2d_nhwc` that records an autograd node when any input requires grad.
    ``relu``: False / True / ``'consumers'`` (see :class:`_ConvFn`); ``mask_input``: ``x`` is the
    output of a ``relu='consumers'`` conv; ``passthrough``: returns ``(y, x_alias)`` — hand ``x_alias``
    to the other consumer of ``x`` (a residual identity path) and the fork's gradient sum rides in
    this conv's dgrad epilogue.  The contract is checked where it can be: outputs of
    ``relu='consumers'`` convs are tagged, and feeding a tagged tensor to a conv WITHOUT
    ``mask_input=True`` raises (its gradient would skip the ReLU gate)."""
    ts = [t for t in (x, w_krsc, bias, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        if x.dtype != torch.float32:
            raise RuntimeError('conv2d_autograd: bf16-stored activations are forward-only (frozen trunk); '
                               'convert to fp32 before a trainable layer')
        if getattr(x, '_bgs_consumers_mask', False) and not mask_input:
            raise RuntimeError("conv2d_autograd: x is the output of a relu='consumers' conv (its ReLU "
                               "backward is delegated to its consumers) but mask_input is False")
        if residual is not None and residual_mode == 0:
            residual_mode = 1
        out = _ConvFn.apply(x, w_krsc, bias, residual, stride, pad, relu, residual_mode,
                            bool(mask_input), bool(passthrough))
        y = out[0] if passthrough else out
        if relu == 'consumers':
            y._bgs_consumers_mask = True
        return out
    y = conv2d_nhwc(x, w_krsc, bias, stride=stride, pad=pad, relu=bool(relu),
                    residual=residual, residual_mode=residual_mode, out_dtype=out_dtype)
    return (y, x) if passthrough else y


def linear(x, weight, bias=None, relu=False, frozen_weight=None):
    """``act(x @ weight.T + bias)`` for ``x [M,K]``, ``weight [Cout,K]`` (nn.Linear layout).
    ``frozen_weight`` (default: ``not weight.requires_grad``, evaluated BEFORE detaching) decides
    whether the bf16 planes of the weight may be cached (see :func:`bfx_split_weights`)."""
    M, K = x.shape
    if frozen_weight is None:
        frozen_weight = not weight.requires_grad
    x = _f32c(x)
    weight = _f32c(weight)
    y = conv2d_nhwc(x.view(M, 1, 1, K), weight.view(weight.shape[0], 1, 1, K),
                    None if bias is None else _f32c(bias), relu=relu, frozen_weight=frozen_weight)
    return y.view(M, weight.shape[0])


class _LinearFn(torch.autograd.Function):
    """y = x @ W^T + b on the fp32 matrix cores, with gradients for x, W, b.

    dW = dY^T X and dX = dY W are the same implicit-GEMM kernel fed with transposed copies
    (both operands must be K-contiguous).  Under selectp=1 only ``fc_cls`` takes this path:
    dW_cls = dlogits^T x is 1.3 GMAC."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return linear(x.detach(), weight.detach(), None if bias is None else bias.detach(),
                      frozen_weight=not weight.requires_grad)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous().float()
        gx = gw = gb = None
        M, K = x.shape
        Nout = weight.shape[0]
        if ctx.needs_input_grad[0]:
            gx = linear(gy, weight.detach().t().contiguous(), frozen_weight=False)   # [M,N] x [K,N]^T
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            # dW[n,k] = sum_m gy[m,n] x[m,k]: the split-reduction wgrad kernel, no transposes
            if Nout % 4 == 0 and K % 4 == 0:
                out = conv2d_wgrad_nhwc(_f32c(x).view(M, 1, 1, K), gy.view(M, 1, 1, Nout), 1,
                                        bias=want_b)
                gw, gb = (out[0], out[1]) if want_b else (out, None)
                gw = gw.view(Nout, K)
            else:
                gw = linear(gy.t().contiguous(), x.detach().t().contiguous(), frozen_weight=False)
                gb = gy.sum(0) if want_b else None
        return gx, gw, gb


def linear_autograd(x, weight, bias=None, relu=False, mask_input=False):
    """``act(x @ weight.T + bias)``: fused forward-only kernel when nothing requires grad,
    otherwise the differentiable path (``relu`` / ``mask_input`` as in :func:`conv2d_autograd`)."""
    needs = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or
                                         (bias is not None and bias.requires_grad))
    if not needs:
        return linear(x, weight, bias, relu=bool(relu))
    M, K = x.shape
    Nout = weight.shape[0]
    y = _ConvFn.apply(x.float().contiguous().view(M, 1, 1, K),
                      weight.float().contiguous().view(Nout, 1, 1, K),
                      None if bias is None else bias.float(), None, 1, 0, relu, 0,
                      bool(mask_input))
    return y.view(M, Nout)


def _grouped_conv3x3_launch(x, w, bias, groups, stride, relu):
    lib = capi.load()
    N, H, W, C = x.shape
    if x.dtype == torch.bfloat16:      # bf16 storage mode: bf16 in, bf16 out (csrc/conv_bf16s.hip)
        out = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=torch.bfloat16,
                          device=x.device)
        rc = lib.bgs_grouped_conv3x3_nhwc_bf16s(capi.ptr(x), capi.ptr(w), capi.ptr(bias), capi.ptr(out),
                                                N, H, W, C, int(groups), int(stride), int(bool(relu)),
                                                capi.current_stream(x.device))
        capi.check('bgs_grouped_conv3x3_nhwc_bf16s', rc)
        return out
    out = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=torch.float32,
                      device=x.device)
    if _CONV_MATH[0] == 'bf16' and stride == 1 and C % 64 == 0:
        # cfg[4] bf16 mode: operands rounded to bf16 in the kernel, fp32 accumulate (the other
        # layouts keep the fp32 kernel: more precise than the mode asks for)
        rc = lib.bgs_grouped_conv3x3_nhwc_bf16ops(capi.ptr(x), capi.ptr(w), capi.ptr(bias),
                                                  capi.ptr(out), N, H, W, C, int(groups), 1,
                                                  int(bool(relu)), capi.current_stream(x.device))
        capi.check('bgs_grouped_conv3x3_nhwc_bf16ops', rc)
        return out
    rc = lib.bgs_grouped_conv3x3_nhwc_f32(capi.ptr(x), capi.ptr(w), capi.ptr(bias), capi.ptr(out),
                                          N, H, W, C, int(groups), int(stride), int(bool(relu)),
                                          capi.current_stream(x.device))
    capi.check('bgs_grouped_conv3x3_nhwc_f32', rc)
    return out


def grouped_dgrad_filter(w, groups):
    """``w [C,3,3,cg]`` -> ``wt[g*cg+cl][2-r][2-s][co_local] = w[g*cg+co_local][r][s][cl]``: the
    filter of the data gradient (transposed inside each group, both spatial axes flipped)."""
    C, _, _, cg = w.shape
    return w.detach().view(groups, cg, 3, 3, cg).flip(2, 3).permute(0, 4, 2, 3, 1) \
        .reshape(C, 3, 3, cg).contiguous()


class _GroupedConvFn(torch.autograd.Function):
    """Differentiable grouped 3x3 conv (+ bias + ReLU): ResNeXt conv2 under ``selectp = 0``
    (resnext.py:47-57).  dx = the MFMA forward kernel on dy with the per-group transposed filter,
    dw / db = ``bgs_grouped_conv3x3_wgrad_nhwc_f32``."""

    @staticmethod
    def forward(ctx, x, w, bias, groups, stride, relu):
        y = _grouped_conv3x3_launch(x.detach(), w.detach(), None if bias is None else bias.detach(),
                                    groups, stride, relu)
        ctx.cfg = (groups, stride, bool(relu), bias is not None)
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        groups, stride, relu, has_bias = ctx.cfg
        lib = capi.load()
        dz = dy.contiguous()
        if relu:
            dz = torch.ops.aten.threshold_backward(dz, y, 0.0)
        N, H, W, C = x.shape
        st = capi.current_stream(x.device)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wt = grouped_dgrad_filter(w, groups)
            dx = torch.empty_like(x)
            rc = lib.bgs_grouped_conv3x3_dgrad_nhwc_f32(capi.ptr(dz), capi.ptr(wt), capi.ptr(dx), N,
                                                        H, W, C, groups, stride, st)
            capi.check('bgs_grouped_conv3x3_dgrad_nhwc_f32', rc)
        want_b = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            dw = torch.empty_like(w)
            db = torch.empty((C,), dtype=torch.float32, device=x.device) if want_b else None
            ws = _workspace(lib.bgs_grouped_conv3x3_wgrad_workspace_bytes(N, H, W, C, groups, stride),
                            x.device)
            rc = lib.bgs_grouped_conv3x3_wgrad_nhwc_f32(capi.ptr(x), capi.ptr(dz), capi.ptr(dw),
                                                        capi.ptr(db), N, H, W, C, groups, stride, 0,
                                                        capi.ptr(ws), st)
            capi.check('bgs_grouped_conv3x3_wgrad_nhwc_f32', rc)
        return dx, dw, db, None, None, None


def grouped_conv3x3_nhwc(x, w, bias, groups, stride=1, relu=False):
    """Grouped 3x3 / pad 1 conv (ResNeXt conv2): x ``[N,H,W,C]``, w ``[C,3,3,C/groups]``; records
    an autograd node when an input requires grad."""
    _require_cuda(x, w, bias)
    assert x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous() and x.dim() == 4
    assert w.is_contiguous() and w.dtype == torch.float32
    N, H, W, C = x.shape
    assert tuple(w.shape) == (C, 3, 3, C // groups), (w.shape, C, groups)
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or
                                    (bias is not None and bias.requires_grad)):
        if x.dtype != torch.float32:
            raise RuntimeError('grouped_conv3x3_nhwc: bf16-stored activations are forward-only')
        return _GroupedConvFn.apply(x, w, bias, int(groups), int(stride), bool(relu))
    return _grouped_conv3x3_launch(x, w, bias, groups, stride, relu)


def _deform_conv3x3_launch(x, offset, w, bias, groups, stride, relu):
    lib = capi.load()
    N, H, W, C = x.shape
    out = torch.empty((N, (H - 1) // stride + 1, (W - 1) // stride + 1, C), dtype=torch.float32,
                      device=x.device)
    rc = lib.bgs_deform_conv3x3_nhwc_f32(capi.ptr(x), capi.ptr(offset), capi.ptr(w), capi.ptr(bias),
                                         capi.ptr(out), N, H, W, C, int(groups), 1, int(offset.shape[3]),
                                         int(stride), int(bool(relu)), capi.current_stream(x.device))
    capi.check('bgs_deform_conv3x3_nhwc_f32', rc)
    return out


class _DeformConvFn(torch.autograd.Function):
    """Differentiable deformable 3x3 conv (+ bias + ReLU), csrc/deform_conv.hip: dx / doffset from one dgrad
    launch (dx by float atomics into a zero-filled map, doffset in a fixed order), dw / db from the
    chunk-reduced wgrad; the ReLU backward and the argument conventions are ``_GroupedConvFn``'s."""

    @staticmethod
    def forward(ctx, x, offset, w, bias, groups, stride, relu):
        y = _deform_conv3x3_launch(x.detach(), offset.detach(), w.detach(),
                                   None if bias is None else bias.detach(), groups, stride, relu)
        ctx.cfg = (groups, stride, bool(relu), bias is not None)
        ctx.save_for_backward(x, offset, w, y if relu else None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, offset, w, y = ctx.saved_tensors
        groups, stride, relu, has_bias = ctx.cfg
        lib = capi.load()
        dz = dy.contiguous()
        if relu:
            dz = torch.ops.aten.threshold_backward(dz, y, 0.0)
        N, H, W, C = x.shape
        pitch = int(offset.shape[3])
        st = capi.current_stream(x.device)
        dx = doff = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None      # the kernel adds into it
            doff = torch.zeros_like(offset) if ctx.needs_input_grad[1] else None  # (padding channels stay 0)
            rc = lib.bgs_deform_conv3x3_dgrad_nhwc_f32(capi.ptr(x), capi.ptr(offset), capi.ptr(w), capi.ptr(dz),
                                                       capi.ptr(dx), capi.ptr(doff), N, H, W, C, groups, 1,
                                                       pitch, stride, st)
            capi.check('bgs_deform_conv3x3_dgrad_nhwc_f32', rc)
        want_b = has_bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2] or want_b:
            dw = torch.empty_like(w)
            db = torch.empty((C,), dtype=torch.float32, device=x.device) if want_b else None
            ws = _workspace(lib.bgs_deform_conv3x3_wgrad_workspace_bytes(N, H, W, C, groups, stride), x.device)
            rc = lib.bgs_deform_conv3x3_wgrad_nhwc_f32(capi.ptr(x), capi.ptr(offset), capi.ptr(dz), capi.ptr(dw),
                                                       capi.ptr(db), N, H, W, C, groups, 1, pitch, stride, 0,
                                                       capi.ptr(ws), st)
            capi.check('bgs_deform_conv3x3_wgrad_nhwc_f32', rc)
        return dx, doff, dw, db, None, None, None


def deform_conv3x3_nhwc(x, offset, w, bias, groups, stride=1, relu=False):
    """Deformable 3x3 / pad 1 conv, DCNv1 with one deformable group (the reference's ``DeformConv``):
    x ``[N,H,W,C]``, offset ``[N,Ho,Wo,pitch >= 18]`` (channel ``2 (3 i + j)`` = dh of tap ``(i, j)``, ``+ 1`` = dw),
    w ``[C,3,3,C/groups]``; records an autograd node when an input requires grad."""
    if x.dtype == torch.bfloat16 or offset.dtype == torch.bfloat16:
        raise NotImplementedError('deform_conv3x3_nhwc: bf16-stored activations have no deformable kernel')
    if _CONV_MATH[0] == 'bf16':
        raise NotImplementedError("deform_conv3x3_nhwc: conv_math='bf16' has no deformable kernel")
    _require_cuda(x, offset, w, bias)
    for t in (x, offset, w) + (() if bias is None else (bias,)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('deform_conv3x3_nhwc: contiguous float32 tensors only')
    if x.dim() != 4 or offset.dim() != 4:
        raise ValueError('deform_conv3x3_nhwc: x [N,H,W,C] and offset [N,Ho,Wo,pitch]')
    N, H, W, C = x.shape
    stride = int(stride)
    if stride not in (1, 2):
        raise NotImplementedError('deform_conv3x3_nhwc: stride %d (1 and 2 have kernels)' % stride)
    if C % groups or tuple(w.shape) != (C, 3, 3, C // groups):
        raise ValueError('deform_conv3x3_nhwc: w must be [C,3,3,C/groups], got %s' % (tuple(w.shape),))
    if C // groups not in (4, 8, 16, 32):
        raise NotImplementedError('deform_conv3x3_nhwc: %d channels per group (4, 8, 16, 32 have kernels)'
                                  % (C // groups))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if tuple(offset.shape[:3]) != (N, Ho, Wo) or offset.shape[3] < 18:
        raise ValueError('deform_conv3x3_nhwc: offset must be [%d,%d,%d,>=18], got %s'
                         % (N, Ho, Wo, tuple(offset.shape)))
    if torch.is_grad_enabled() and (x.requires_grad or offset.requires_grad or w.requires_grad or
                                    (bias is not None and bias.requires_grad)):
        return _DeformConvFn.apply(x, offset, w, bias, int(groups), stride, bool(relu))
    return _deform_conv3x3_launch(x, offset, w, bias, groups, stride, relu)


def nchw_to_nhwc4(img):
    """``[N, C <= 4, H, W]`` image batch -> ``[N, H, W, 4]`` fp32, channels zero-padded (the stem conv's
    16-byte pixels) in one launch (``bgs_nchw_to_nhwc4_f32``)."""
    _require_cuda(img)
    lib = capi.load()
    x = img.detach().to(torch.float32).contiguous()
    N, C, H, W = x.shape
    out = torch.empty((N, H, W, 4), dtype=torch.float32, device=x.device)
    rc = lib.bgs_nchw_to_nhwc4_f32(capi.ptr(x), capi.ptr(out), N, C, H, W, capi.current_stream(x.device))
    capi.check('bgs_nchw_to_nhwc4_f32', rc)
    return out


def stem_fused_enabled():
    """The one-launch stem (conv 7x7 / s2 + ReLU + max-pool from the NCHW image, csrc/stem_fused.hip):
    ``BGS_STEM_FUSED=0`` keeps the three-launch chain (A/B; read at every call)."""
    return os.environ.get('BGS_STEM_FUSED', '1') != '0' and _CONV_MATH[0] == 'bf16x6'


def stem_fused_split_weights(w_krsc):
    """Folded stem filter ``[64, 7, 7, >=3]`` -> the split planes ``bgs_stem_conv7x7s2_relu_maxpool_nchw_f32`` reads."""
    _require_cuda(w_krsc)
    lib = capi.load()
    w = _f32c(w_krsc)
    assert w.dim() == 4 and tuple(w.shape[:3]) == (64, 7, 7) and w.shape[3] >= 3, tuple(w.shape)
    out = torch.empty(lib.bgs_stem_fused_weight_bytes(), dtype=torch.uint8, device=w.device)
    rc = lib.bgs_stem_fused_split_weights(capi.ptr(w), int(w.shape[3]), capi.ptr(out), capi.current_stream(w.device))
    capi.check('bgs_stem_fused_split_weights', rc)
    return out


def stem_fused(img, wsplit, bias):
    """``relu(conv7x7s2(img) + bias)`` max-pooled 3x3 / s2 / p1 in ONE launch: ``img [N, 3, H, W]`` (NCHW, as the
    reference hands it over) -> ``[N, PH, PW, 64]`` NHWC fp32.  Forward only (the frozen stem of the BAGS configs)."""
    _require_cuda(img, wsplit, bias)
    lib = capi.load()
    x = img.detach().to(torch.float32).contiguous()
    N, C, H, W = x.shape
    assert C == 3
    CH, CW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (CH - 1) // 2 + 1, (CW - 1) // 2 + 1
    out = torch.empty((N, PH, PW, 64), dtype=torch.float32, device=x.device)
    rc = lib.bgs_stem_conv7x7s2_relu_maxpool_nchw_f32(capi.ptr(x), capi.ptr(wsplit), capi.ptr(_f32c(bias)),
                                                      capi.ptr(out), N, H, W, capi.current_stream(x.device))
    capi.check('bgs_stem_conv7x7s2_relu_maxpool_nchw_f32', rc)
    return out


def _maxpool_launch(x, out_dtype=torch.float32):
    lib = capi.load()
    N, H, W, C = x.shape
    if out_dtype == torch.bfloat16:    # entry of the bf16-stored trunk
        out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.bfloat16, device=x.device)
        rc = lib.bgs_maxpool3x3s2_nhwc_f32_to_bf16(capi.ptr(x), capi.ptr(out), N, H, W, C,
                                                   capi.current_stream(x.device))
        capi.check('bgs_maxpool3x3s2_nhwc_f32_to_bf16', rc)
        return out
    out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32,
                      device=x.device)
    rc = lib.bgs_maxpool3x3s2_nhwc_f32(capi.ptr(x), capi.ptr(out), N, H, W, C,
                                       capi.current_stream(x.device))
    capi.check('bgs_maxpool3x3s2_nhwc_f32', rc)
    return out


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _maxpool_launch(x.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        lib = capi.load()
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        rc = lib.bgs_maxpool3x3s2_bwd_nhwc_f32(capi.ptr(x), capi.ptr(dy.contiguous()), capi.ptr(dx),
                                               N, H, W, C, capi.current_stream(x.device))
        capi.check('bgs_maxpool3x3s2_bwd_nhwc_f32', rc)
        return dx


def maxpool3x3s2_nhwc(x, out_dtype=torch.float32):
    """3x3 / stride 2 / pad 1 max pooling (ResNet stem); differentiable when ``x`` requires grad
    (``frozen_stages < 1``).  ``out_dtype=torch.bfloat16``: the pooled map is stored in bf16."""
    _require_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    if torch.is_grad_enabled() and x.requires_grad:
        assert out_dtype == torch.float32
        return _MaxPoolFn.apply(x)
    return _maxpool_launch(x, out_dtype)


# ----------------------------------------------------------------------------------------
# RoIAlign (multi-level, NHWC) and batched NMS
# ----------------------------------------------------------------------------------------
def roi_align_nhwc(feats, rois, featmap_strides, out_size=7, sample_num=2, finest_scale=56,
                   return_levels=False, pool=1, out=None):
    """feats: list of ``[N,H_l,W_l,C]`` maps; rois ``[K,5]`` -> ``[K, out, out, C]``.
    ``pool``: RoIAlign on the ``(out*pool)^2`` grid averaged down to ``out^2`` in the kernel
    (== ``F.adaptive_avg_pool2d`` of the finer result);  ``out``: accumulate INTO this tensor."""
    import ctypes
    _require_cuda(rois, *feats)
    lib = capi.load()
    L = len(feats)
    N, _, _, C = feats[0].shape
    for f in feats:
        assert f.dtype == torch.float32 and f.is_contiguous() and f.shape[0] == N and f.shape[3] == C
    rois = _f32c(rois)
    K = rois.shape[0]
    ph, pw = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
    accumulate = out is not None
    if accumulate:
        assert tuple(out.shape) == (K, ph, pw, C) and out.is_contiguous() and \
            out.dtype == torch.float32, (out.shape, (K, ph, pw, C))
    else:
        out = torch.empty((K, ph, pw, C), dtype=torch.float32, device=rois.device)
    lv = torch.empty((K,), dtype=torch.int32, device=rois.device) if return_levels else None
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hs = (ctypes.c_int * L)(*[int(f.shape[1]) for f in feats])
    ws = (ctypes.c_int * L)(*[int(f.shape[2]) for f in feats])
    sc = (ctypes.c_float * L)(*[1.0 / s for s in featmap_strides])
    rc = lib.bgs_roi_align_nhwc_fwd_ex(ptrs, hs, ws, sc, L, N, float(finest_scale), capi.ptr(rois),
                                       K, C, ph, pw, sample_num, int(pool), int(accumulate),
                                       capi.ptr(out), capi.ptr(lv),
                                       capi.current_stream(rois.device))
    capi.check('bgs_roi_align_nhwc_fwd_ex', rc)
    return (out, lv) if return_levels else out


def roi_align_nhwc_bwd(dout, rois, dfeats, featmap_strides, sample_num=2, finest_scale=56, pool=1):
    """Scatter ``dout [K,ph,pw,C]`` into the per-level gradient maps ``dfeats`` (accumulated
    into, in place, with fp32 atomics)."""
    import ctypes
    _require_cuda(dout, rois, *dfeats)
    lib = capi.load()
    L = len(dfeats)
    N, _, _, C = dfeats[0].shape
    for f in dfeats:
        assert f.dtype == torch.float32 and f.is_contiguous() and f.shape[0] == N and f.shape[3] == C
    rois = _f32c(rois)
    dout = _f32c(dout)
    K, ph, pw, C2 = dout.shape
    assert C2 == C and rois.shape[0] == K
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in dfeats])
    hs = (ctypes.c_int * L)(*[int(f.shape[1]) for f in dfeats])
    ws = (ctypes.c_int * L)(*[int(f.shape[2]) for f in dfeats])
    sc = (ctypes.c_float * L)(*[1.0 / s for s in featmap_strides])
    rc = lib.bgs_roi_align_nhwc_bwd_ex(ptrs, hs, ws, sc, L, N, float(finest_scale), capi.ptr(rois),
                                       K, C, ph, pw, sample_num, int(pool), capi.ptr(dout),
                                       capi.current_stream(rois.device))
    capi.check('bgs_roi_align_nhwc_bwd_ex', rc)
    return dfeats


class _RoIAlignFn(torch.autograd.Function):
    """Differentiable multi-level RoIAlign (w.r.t. the feature maps; RoIs carry no gradient, as
    in the reference: roi_align.py:52).  With ``base`` the pooled result is added into it in
    place (HTC semantic fusion: ``bbox_feats += pooled_semantic``); its gradient is ``dout``."""

    @staticmethod
    def forward(ctx, rois, strides, out_size, sample_num, finest_scale, pool, base, *feats):
        ctx.save_for_backward(rois)
        ctx.cfg = (tuple(strides), sample_num, finest_scale, pool, [tuple(f.shape) for f in feats],
                   base is not None)
        if base is not None:
            ctx.mark_dirty(base)
        return roi_align_nhwc([f.detach() for f in feats], rois, strides, out_size, sample_num,
                              finest_scale, pool=pool, out=base)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        rois, = ctx.saved_tensors
        strides, sample_num, finest_scale, pool, shapes, has_base = ctx.cfg
        dout = dout.contiguous()
        dfeats = [None] * len(shapes)
        if any(ctx.needs_input_grad[7:]):
            dfeats = [torch.zeros(s, dtype=torch.float32, device=dout.device) for s in shapes]
            roi_align_nhwc_bwd(dout, rois, dfeats, strides, sample_num, finest_scale, pool=pool)
        dbase = dout if has_base and ctx.needs_input_grad[6] else None
        return (None, None, None, None, None, None, dbase) + tuple(dfeats)


def roi_align_nhwc_autograd(feats, rois, featmap_strides, out_size=7, sample_num=2,
                            finest_scale=56, pool=1, add_to=None):
    """``add_to``: RoI features ``[K, out, out, C]`` that receive ``+= pooled`` in place."""
    ts = list(feats) + ([add_to] if add_to is not None else [])
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return _RoIAlignFn.apply(rois, tuple(featmap_strides), out_size, sample_num, finest_scale,
                                 pool, add_to, *feats)
    return roi_align_nhwc(feats, rois, featmap_strides, out_size, sample_num, finest_scale,
                          pool=pool, out=add_to)


def resize_bilinear_nhwc(x, size):
    """``F.interpolate(x, size, mode='bilinear', align_corners=True)`` on an NHWC map."""
    _require_cuda(x)
    lib = capi.load()
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    N, H, W, C = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
    rc = lib.bgs_resize_bilinear_nhwc_f32(capi.ptr(x), capi.ptr(y), N, H, W, C, Ho, Wo, 1,
                                          capi.current_stream(x.device))
    capi.check('bgs_resize_bilinear_nhwc_f32', rc)
    return y


class _ResizeBilinearFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, size):
        ctx.in_shape = tuple(x.shape)
        return resize_bilinear_nhwc(x.detach(), size)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        lib = capi.load()
        N, H, W, C = ctx.in_shape
        dy = dy.contiguous()
        dx = torch.zeros(ctx.in_shape, dtype=torch.float32, device=dy.device)
        rc = lib.bgs_resize_bilinear_nhwc_bwd_f32(capi.ptr(dy), capi.ptr(dx), N, H, W, C,
                                                  dy.shape[1], dy.shape[2], 1,
                                                  capi.current_stream(dy.device))
        capi.check('bgs_resize_bilinear_nhwc_bwd_f32', rc)
        return dx, None


def resize_bilinear_nhwc_autograd(x, size):
    if torch.is_grad_enabled() and x.requires_grad:
        return _ResizeBilinearFn.apply(x, tuple(size))
    return resize_bilinear_nhwc(x, size)


def topk_sorted(rows, ks, kmax, inner=None):
    """Sorted top-k of several row sets in one launch set (``bgs_topk_sorted_f32``).

    ``rows``: list of L float32 tensors, one per set, ``[N, ...]`` with contiguous per-image
    blocks; ``ks``: list of L ints (``k_l <= kmax <= 4096``).  ``inner=None``: each per-image
    block is a flat row.  ``inner=A``: the block is ``[n_pix, C]`` and the row consists of the
    FIRST ``A`` channels of every pixel (``n_pix * A`` elements, index ``pix * A + a``) — the
    objectness logits inside the fused RPN head output, read in place.
    Returns ``(values, indices)`` ``[N, L, kmax]``: per (image, set) the ``min(k_l, len)`` largest
    entries in descending order and their row positions, zeros beyond.  ``N * L <= 64``."""
    import ctypes
    _require_cuda(*rows)
    lib = capi.load()
    N = rows[0].shape[0]
    L = len(rows)
    dev = rows[0].device
    ptrs, lens, kk, inn, pit = [], [], [], [], []
    for i in range(N):
        for r, k in zip(rows, ks):
            assert r.shape[0] == N and r.dtype == torch.float32 and r.is_contiguous()
            per = r[0].numel()
            ptrs.append(r.data_ptr() + i * per * 4)
            if inner is None:
                lens.append(per)
                inn.append(0)
                pit.append(0)
            else:
                C = int(r.shape[-1])
                lens.append(per // C * int(inner))
                inn.append(int(inner))
                pit.append(C)
            kk.append(int(k))
    P = N * L
    vals = torch.empty((N, L, kmax), dtype=torch.float32, device=dev)
    idx = torch.empty((N, L, kmax), dtype=torch.int64, device=dev)
    ws = _workspace(lib.bgs_topk_workspace_bytes(P, int(kmax)), dev)
    rc = lib.bgs_topk_sorted_f32((ctypes.c_void_p * P)(*ptrs), _c_int_array(lens), _c_int_array(kk),
                                 _c_int_array(inn) if inner is not None else None,
                                 _c_int_array(pit) if inner is not None else None,
                                 P, int(kmax), capi.ptr(vals), capi.ptr(idx), capi.ptr(ws),
                                 capi.current_stream(dev))
    capi.check('bgs_topk_sorted_f32', rc)
    return vals, idx


def nms_batched(boxes, counts, iou_thr, iou_mode=0, max_keep=0):
    """boxes ``[P,nmax,5]`` sorted by descending score per problem, counts ``[P]`` i32 ->
    ``keep [P,nmax]`` i32 (ascending indices), ``keep_count [P]`` i32.  No host sync."""
    _require_cuda(boxes, counts)
    lib = capi.load()
    boxes = _f32c(boxes)
    assert boxes.dim() == 3 and boxes.shape[2] == 5 and counts.dtype == torch.int32
    P, nmax, _ = boxes.shape
    dev = boxes.device
    keep = torch.empty((P, nmax), dtype=torch.int32, device=dev)
    keep_count = torch.empty((P,), dtype=torch.int32, device=dev)
    ws = _workspace(lib.bgs_nms_workspace_bytes(P, nmax), dev)
    rc = lib.bgs_nms_batched(capi.ptr(boxes), capi.ptr(counts), P, nmax, float(iou_thr),
                             int(iou_mode), int(max_keep), capi.ptr(keep), capi.ptr(keep_count),
                             capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_nms_batched', rc)
    return keep, keep_count


SOFT_NMS_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}


def soft_nms_batched(dets, counts, iou_thr, method='linear', sigma=0.5, min_score=1e-3):
    """dets ``[P,nmax,5]`` in candidate order per problem, counts ``[P]`` i32 -> ``order [P,nmax]`` i32 (candidate
    indices in selection order), ``scores [P,nmax]`` f32 (decayed score at selection), ``keep_count [P]`` i32
    (``bgs_soft_nms_batched``: one launch, no host sync).  ``method``: ``'linear'`` / ``'gaussian'`` / ``'hard'``
    or its code 1 / 2 / 0."""
    _require_cuda(dets, counts)
    code = SOFT_NMS_METHODS.get(method, method)
    if code not in (0, 1, 2):
        raise ValueError('Invalid method for SoftNMS: {}'.format(method))
    lib = capi.load()
    dets = _f32c(dets)
    assert dets.dim() == 3 and dets.shape[2] == 5 and counts.dtype == torch.int32
    P, nmax, _ = dets.shape
    dev = dets.device
    order = torch.empty((P, nmax), dtype=torch.int32, device=dev)
    scores = torch.empty((P, nmax), dtype=torch.float32, device=dev)
    keep_count = torch.empty((P,), dtype=torch.int32, device=dev)
    rc = lib.bgs_soft_nms_batched(capi.ptr(dets), capi.ptr(counts.contiguous()), P, nmax, float(iou_thr), int(code),
                                  float(sigma), float(min_score), capi.ptr(order), capi.ptr(scores),
                                  capi.ptr(keep_count), capi.current_stream(dev))
    capi.check('bgs_soft_nms_batched', rc)
    return order, scores, keep_count


DET_CANDIDATE_MODES = {'sorted': 0, 'original': 1}
DET_SELECT_WORKSPACE_PER_IMAGE = 65536


def det_candidates(scores, boxes, score_thr, mode='sorted', valid=None, score_factors=None, out=None):
    """The candidate lists of all ``B * (C - 1)`` (image, class) problems in ONE launch (``bgs_det_candidates``).
    scores ``[B,n,C]`` f32 (column 0 = background), boxes ``[B,n,4C]`` or ``[B,n,4]`` f32 (decoded), valid
    ``[B,n]`` bool / uint8, score_factors ``[B,n]`` -> ``dets [B*(C-1),n,5]``, ``idx [B*(C-1),n]`` i32 (row
    inside the image), ``counts [B*(C-1)]`` i32.  ``mode='sorted'``: the rows with raw score ``> score_thr`` by
    descending score x factor, ties by ascending row (hard NMS); ``'original'``: in row order (soft-NMS).  Slots
    past the count are zero, ``idx`` -1.  ``n <= 4096``.  No host sync."""
    _require_cuda(scores, boxes, valid, score_factors)
    code = DET_CANDIDATE_MODES.get(mode, mode)
    if code not in (0, 1):
        raise ValueError('det_candidates: mode must be "sorted" or "original" (got %r)' % (mode,))
    lib = capi.load()
    assert scores.dim() == 3 and boxes.dim() == 3 and scores.dtype == torch.float32 and boxes.dtype == torch.float32
    B, n, C = scores.shape
    assert boxes.shape[:2] == (B, n) and boxes.shape[2] in (4, 4 * C) and C >= 2 and n >= 1 and B >= 1
    scores, boxes = scores.detach().contiguous(), boxes.detach().contiguous()
    if valid is not None:
        assert valid.shape == (B, n) and valid.dtype in (torch.bool, torch.uint8)
        valid = valid.contiguous().view(torch.uint8)
    if score_factors is not None:
        assert score_factors.shape == (B, n)
        score_factors = _f32c(score_factors)
    dev = scores.device
    P = B * (C - 1)
    if out is None:
        out = (torch.empty((P, n, 5), dtype=torch.float32, device=dev),
               torch.empty((P, n), dtype=torch.int32, device=dev),
               torch.empty((P,), dtype=torch.int32, device=dev))
    dets, idx, counts = out
    assert dets.shape == (P, n, 5) and dets.dtype == torch.float32 and dets.is_contiguous()
    assert idx.shape == (P, n) and idx.dtype == torch.int32 and idx.is_contiguous()
    assert counts.shape == (P,) and counts.dtype == torch.int32
    rc = lib.bgs_det_candidates(capi.ptr(scores), capi.ptr(boxes), capi.ptr(valid) if valid is not None else None,
                                capi.ptr(score_factors) if score_factors is not None else None, B, n, C,
                                int(boxes.shape[2]), float(score_thr), int(code), capi.ptr(dets), capi.ptr(idx),
                                capi.ptr(counts), capi.current_stream(dev))
    capi.check('bgs_det_candidates', rc)
    return dets, idx, counts


def det_select(dets, idx, keep, keep_count, num_imgs, max_num, sel_scores=None, out=None):
    """The final fixed-shape detections of ``num_imgs`` images (``bgs_det_select``: two launches whatever the batch,
    no host sync).  ``dets [P,n,5]`` / ``idx [P,n]`` of :func:`det_candidates`, ``keep`` / ``keep_count`` of
    :func:`nms_batched`, or ``order`` / ``keep_count`` and ``sel_scores`` of :func:`soft_nms_batched`;
    ``P = num_imgs * (C - 1)`` -> ``out_dets [B,max_num,5]``, ``out_labels [B,max_num]`` i32 (0-based, -1 in the
    unused slots), ``out_count [B]`` i32.  Nothing cut: class-major (hard: ascending original row inside a class,
    soft: selection order); cut: by descending score, ties in class-major concatenation order.
    ``max_num <= min(n * (C - 1), 4096)``."""
    _require_cuda(dets, idx, keep, keep_count, sel_scores)
    lib = capi.load()
    assert dets.dim() == 3 and dets.shape[2] == 5 and dets.dtype == torch.float32 and dets.is_contiguous()
    P, n, _ = dets.shape
    B = int(num_imgs)
    assert B >= 1 and P % B == 0 and int(max_num) > 0
    for t in (idx, keep):
        assert t.shape == (P, n) and t.dtype == torch.int32 and t.is_contiguous()
    assert keep_count.shape == (P,) and keep_count.dtype == torch.int32
    if sel_scores is not None:
        assert sel_scores.shape == (P, n) and sel_scores.dtype == torch.float32 and sel_scores.is_contiguous()
    dev = dets.device
    max_num = int(max_num)
    if out is None:
        out = (torch.empty((B, max_num, 5), dtype=torch.float32, device=dev),
               torch.empty((B, max_num), dtype=torch.int32, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev))
    out_dets, out_labels, out_count = out
    assert out_dets.shape == (B, max_num, 5) and out_dets.dtype == torch.float32 and out_dets.is_contiguous()
    assert out_labels.shape == (B, max_num) and out_labels.dtype == torch.int32 and out_labels.is_contiguous()
    assert out_count.shape == (B,) and out_count.dtype == torch.int32
    ws = _workspace(B * DET_SELECT_WORKSPACE_PER_IMAGE, dev)
    rc = lib.bgs_det_select(capi.ptr(dets), capi.ptr(idx), capi.ptr(keep),
                            capi.ptr(sel_scores) if sel_scores is not None else None,
                            capi.ptr(keep_count.contiguous()), B, P // B, n, max_num, capi.ptr(out_dets),
                            capi.ptr(out_labels), capi.ptr(out_count), capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_det_select', rc)
    return out_dets, out_labels, out_count


def nms_gather(boxes, keep, keep_count):
    """``boxes [R,nmax,5]``, ``keep [R,nmax]`` / ``keep_count [R]`` of :func:`nms_batched` ->
    ``(kept [R,nmax,5], scores [R,nmax])``: the kept boxes in fixed-shape rows, score -1 in the slots
    past ``keep_count`` (``bgs_nms_gather``: one launch)."""
    _require_cuda(boxes, keep, keep_count)
    lib = capi.load()
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 3 and boxes.shape[2] == 5
    assert keep.dtype == torch.int32 and keep.is_contiguous() and keep_count.dtype == torch.int32
    R, nmax, _ = boxes.shape
    out = torch.empty_like(boxes)
    sc = torch.empty((R, nmax), dtype=torch.float32, device=boxes.device)
    rc = lib.bgs_nms_gather(capi.ptr(boxes), capi.ptr(keep), capi.ptr(keep_count.contiguous()), R, nmax,
                            capi.ptr(out), capi.ptr(sc), capi.current_stream(boxes.device))
    capi.check('bgs_nms_gather', rc)
    return out, sc


def nms_merge_select(boxes, keep, keep_count, num_images, num, out=None):
    """The proposal tail in one launch (``bgs_nms_merge_select``): ``boxes [N*L,nmax,5]`` (rows sorted by
    descending score), ``keep`` / ``keep_count`` of :func:`nms_batched` -> ``(props [N,num,5], valid [N,num] bool)``:
    the ``num`` best kept boxes of each image over its L levels, in descending score order.  Every slot is
    written (ranks are a permutation under the kernel's total order; the slots past the kept total are zeroed).
    ``out``: optional pre-allocated ``(props f32, valid u8)`` pair (tests poison it to prove full coverage)."""
    _require_cuda(boxes, keep, keep_count)
    lib = capi.load()
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.dim() == 3 and boxes.shape[2] == 5
    assert keep.dtype == torch.int32 and keep.is_contiguous() and keep_count.dtype == torch.int32
    R, nmax, _ = boxes.shape
    N = int(num_images)
    assert R % N == 0
    if out is None:
        props = torch.empty((N, int(num), 5), dtype=torch.float32, device=boxes.device)
        valid = torch.empty((N, int(num)), dtype=torch.uint8, device=boxes.device)
    else:
        props, valid = out
        assert props.shape == (N, int(num), 5) and props.dtype == torch.float32 and props.is_contiguous()
        assert valid.shape == (N, int(num)) and valid.dtype == torch.uint8 and valid.is_contiguous()
    rc = lib.bgs_nms_merge_select(capi.ptr(boxes), capi.ptr(keep), capi.ptr(keep_count.contiguous()), N, R // N,
                                  nmax, int(num), capi.ptr(props), capi.ptr(valid),
                                  capi.current_stream(boxes.device))
    capi.check('bgs_nms_merge_select', rc)
    return props, valid.view(torch.bool)


def gather_boxes(flat, idx, scores):
    """``props [N,num,5] = flat[n, idx[n,j]]``, ``valid [N,num] (bool) = scores >= 0``
    (``bgs_gather_boxes``: one launch)."""
    _require_cuda(flat, idx, scores)
    lib = capi.load()
    assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.dim() == 3 and flat.shape[2] == 5
    assert idx.dtype == torch.int64 and idx.is_contiguous() and scores.dtype == torch.float32 \
        and scores.is_contiguous() and idx.shape == scores.shape
    N, T, _ = flat.shape
    num = idx.shape[1]
    props = torch.empty((N, num, 5), dtype=torch.float32, device=flat.device)
    valid = torch.empty((N, num), dtype=torch.uint8, device=flat.device)
    rc = lib.bgs_gather_boxes(capi.ptr(flat), capi.ptr(idx), capi.ptr(scores), N, T, num, capi.ptr(props),
                              capi.ptr(valid), capi.current_stream(flat.device))
    capi.check('bgs_gather_boxes', rc)
    return props, valid.view(torch.bool)


# ----------------------------------------------------------------------------------------
# test-time augmentation: box mapping and the merges of aug_test (csrc/aug_merge.hip)
# ----------------------------------------------------------------------------------------
AUG_MAX_VIEWS = 16
AUG_MAX_MASK_ENTRIES = 64
_AUG_MAP_MODES = {'boxes': 0, 'rois': 1, 'nms': 2}


def _aug_geoms(geoms):
    """``[(scale_factor, flip, W), ...]`` -> the three HOST arrays of the C ABI."""
    for s, _, _ in geoms:
        if not isinstance(s, float):
            raise NotImplementedError('aug_test takes a float scale_factor (keep_ratio=True); got %r' % (s,))
    return (_c_float_array([g[0] for g in geoms]), _c_int_array([1 if g[1] else 0 for g in geoms]),
            _c_int_array([int(g[2]) for g in geoms]))


def aug_map_boxes(srcs, geoms, back=False, mode='boxes', valids=None):
    """``bbox_mapping`` / ``bbox_mapping_back`` for A views in one launch (``bgs_aug_map_boxes``).

    ``srcs``: A float32 ``[n, cols]`` tensors (the same tensor A times maps one set into every view) whose first
    ``4 * nbox`` columns are boxes; ``geoms``: A ``(scale_factor, flip, W)`` triples.
    ``mode='boxes'``: ``[A, n, 4 * nbox]`` (``nbox = cols // 4``); ``'rois'``: ``[A, n, 5]`` rows ``(0, box)``;
    ``'nms'`` (``cols == 5``): ``(rows [A * n, 5], scores [A * n], count [1] int32)`` — the concatenated proposals of
    ``merge_aug_proposals`` with score -1 in the rows whose ``valids[a]`` entry is False."""
    _require_cuda(*srcs)
    A = len(srcs)
    if A != len(geoms) or A == 0:
        raise ValueError('one (scale_factor, flip, W) triple per view')
    if A > AUG_MAX_VIEWS:
        raise NotImplementedError('bgs_aug_map_boxes: at most %d views (got %d)' % (AUG_MAX_VIEWS, A))
    code = _AUG_MAP_MODES[mode]
    srcs = [s if s.dtype == torch.float32 and s.is_contiguous() else _f32c(s) for s in srcs]
    n, cols = srcs[0].shape
    assert all(s.shape == (n, cols) for s in srcs)
    dev = srcs[0].device
    nbox = cols // 4 if code == 0 else 1
    out_scores = count = None
    if code == 0:
        out = torch.empty((A, n, 4 * nbox), dtype=torch.float32, device=dev)
    elif code == 1:
        out = torch.empty((A, n, 5), dtype=torch.float32, device=dev)
    else:
        assert cols == 5
        if A * n > 4096:
            raise NotImplementedError('merged proposals: A x max_num <= 4096 (bgs_nms_batched); got %d' % (A * n))
        out = torch.empty((A * n, 5), dtype=torch.float32, device=dev)
        out_scores = torch.empty((A * n,), dtype=torch.float32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
    vals = None
    if valids is not None:
        valids = [v.view(torch.uint8) if v.dtype == torch.bool else v.to(torch.uint8) for v in valids]
        valids = [v.contiguous() for v in valids]
        assert len(valids) == A and all(v.numel() == n for v in valids)
        _require_cuda(*valids)
        vals = _c_ptr_array(valids)
    sc, fl, wd = _aug_geoms(geoms)
    rc = capi.load().bgs_aug_map_boxes(_c_ptr_array(srcs), vals, A, n, cols, nbox, sc, fl, wd, 1 if back else 0,
                                       code, capi.ptr(out), None if out_scores is None else capi.ptr(out_scores),
                                       None if count is None else capi.ptr(count), capi.current_stream(dev))
    capi.check('bgs_aug_map_boxes', rc)
    if code == 2:
        return out, out_scores, count
    return out


def _aligned(t):
    t = t if t.dtype == torch.float32 and t.is_contiguous() else _f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def aug_merge_bboxes(boxes, scores, geoms, valid=None):
    """``merge_aug_bboxes`` in one launch (``bgs_aug_merge_bboxes``): A views of ``boxes [n, 4k]`` (view scale, not
    yet mapped back) and ``scores [n, C]`` -> ``(mean of the mapped-back boxes, mean of the scores)``; sums in view
    order, then / A.  ``valid [n]``: rows where it is False get score -1 (the padding of the proposal list)."""
    _require_cuda(*boxes, *scores)
    A = len(boxes)
    if A != len(scores) or A != len(geoms) or A == 0:
        raise ValueError('one boxes / scores / (scale_factor, flip, W) per view')
    if A > AUG_MAX_VIEWS:
        raise NotImplementedError('bgs_aug_merge_bboxes: at most %d views (got %d)' % (AUG_MAX_VIEWS, A))
    boxes = [_aligned(b) for b in boxes]
    scores = [_aligned(s) for s in scores]
    n, bc = boxes[0].shape
    C = scores[0].shape[1]
    assert all(b.shape == (n, bc) for b in boxes) and all(s.shape == (n, C) for s in scores)
    dev = boxes[0].device
    out_b = torch.empty((n, bc), dtype=torch.float32, device=dev)
    out_s = torch.empty((n, C), dtype=torch.float32, device=dev)
    if valid is not None:
        valid = (valid.view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)).contiguous()
        assert valid.numel() == n
    sc, fl, wd = _aug_geoms(geoms)
    rc = capi.load().bgs_aug_merge_bboxes(_c_ptr_array(boxes), _c_ptr_array(scores), A, n, bc, C, sc, fl, wd,
                                          None if valid is None else capi.ptr(valid), capi.ptr(out_b),
                                          capi.ptr(out_s), capi.current_stream(dev))
    capi.check('bgs_aug_merge_bboxes', rc)
    return out_b, out_s


def aug_merge_masks(masks, flips):
    """``merge_aug_masks`` without weights in one launch (``bgs_aug_merge_masks``): M ``[k, 28, 28]`` probability
    tensors, entry m mirrored along x where ``flips[m]`` -> their mean (sum in entry order, then / M)."""
    _require_cuda(*masks)
    M = len(masks)
    if M != len(flips) or M == 0:
        raise ValueError('one flip flag per mask entry')
    if M > AUG_MAX_MASK_ENTRIES:
        raise NotImplementedError('bgs_aug_merge_masks: at most %d entries (got %d)' % (AUG_MAX_MASK_ENTRIES, M))
    masks = [_aligned(m) for m in masks]
    k, S, S2 = masks[0].shape
    assert S == S2 and all(m.shape == (k, S, S) for m in masks)
    out = torch.empty((k, S, S), dtype=torch.float32, device=masks[0].device)
    rc = capi.load().bgs_aug_merge_masks(_c_ptr_array(masks), _c_int_array([1 if f else 0 for f in flips]), M, k, S,
                                         capi.ptr(out), capi.current_stream(masks[0].device))
    capi.check('bgs_aug_merge_masks', rc)
    return out


# ----------------------------------------------------------------------------------------
# fused target assignment / RPN loss / proposal decode / RoI targets (csrc/det_targets.hip)
# ----------------------------------------------------------------------------------------
def _c_int_array(vals):
    import ctypes
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _c_float_array(vals):
    import ctypes
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def _c_ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def iou_assign(boxes, gt_cat, gt_offsets, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, valid=None,
               shared_boxes=False, return_max_overlaps=False):
    """``MaxIoUAssigner`` for N images at once -> ``assigned [N,A]`` int32.

    boxes: ``[A, >=4]`` with ``shared_boxes=True`` (the same anchors for every image) or
    ``[N, A, >=4]``; gt_cat ``[sum G, 4]`` with python ``gt_offsets`` (len N+1); valid ``[N,A]`` u8."""
    _require_cuda(boxes, gt_cat, valid)
    lib = capi.load()
    boxes = boxes if boxes.dtype == torch.float32 and boxes.is_contiguous() else _f32c(boxes)
    gt_cat = _f32c(gt_cat)
    N = len(gt_offsets) - 1
    for i in range(N):
        # max_iou_assigner.py:76-77: an image without GT boxes is an error in the reference; the
        # fused kernel would silently mark every box of that image "ignore" (-1)
        if gt_offsets[i + 1] - gt_offsets[i] <= 0:
            raise ValueError('No gt or proposals (image %d of the batch has no GT box)' % i)
    if shared_boxes:
        A, bs = boxes.shape[0], boxes.shape[1]
        img_stride = 0
    else:
        assert boxes.shape[0] == N
        A, bs = boxes.shape[1], boxes.shape[2]
        img_stride = A * bs
    if isinstance(neg_iou_thr, (tuple, list)):
        lo, hi = neg_iou_thr
    else:
        lo, hi = 0.0, neg_iou_thr
    dev = boxes.device
    if valid is not None:
        assert valid.dtype == torch.uint8 and tuple(valid.shape) == (N, A) and valid.is_contiguous()
    assigned = torch.empty((N, A), dtype=torch.int32, device=dev)
    mo = torch.empty((N, A), dtype=torch.float32, device=dev) if return_max_overlaps else None
    ws = _workspace(lib.bgs_iou_assign_workspace_bytes(N, A, int(gt_offsets[-1])), dev)
    rc = lib.bgs_iou_assign(capi.ptr(boxes), img_stride, bs, capi.ptr(valid), capi.ptr(gt_cat),
                            _c_int_array(gt_offsets), N, A, float(pos_iou_thr), float(lo),
                            float(hi), float(min_pos_iou), capi.ptr(assigned), capi.ptr(mo),
                            capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_iou_assign', rc)
    return (assigned, mo) if return_max_overlaps else assigned


def _rpn_loss_launch(level_outs, num_anchors, anchors, assigned, pos_mask, neg_mask, gt_cat,
                     gt_offsets, means, stds, beta, pos_weight, loss_weight_cls, loss_weight_bbox):
    lib = capi.load()
    L = len(level_outs)
    N = level_outs[0].shape[0]
    for o in level_outs:
        assert o.dtype == torch.float32 and o.is_contiguous() and o.shape[-1] == 5 * num_anchors
    hw = [int(o.shape[1] * o.shape[2]) for o in level_outs]
    A = sum(hw) * num_anchors
    assert tuple(assigned.shape) == (N, A) and assigned.dtype == torch.int32
    assert pos_mask.dtype == torch.uint8 and neg_mask.dtype == torch.uint8
    assert anchors.shape == (A, 4) and anchors.is_contiguous()
    dev = anchors.device
    lc = torch.empty((L,), dtype=torch.float32, device=dev)
    lb = torch.empty((L,), dtype=torch.float32, device=dev)
    nt = torch.empty((1,), dtype=torch.float32, device=dev)
    ws = _workspace(lib.bgs_rpn_loss_workspace_bytes(N, A, L), dev)
    rc = lib.bgs_rpn_loss(_c_ptr_array(level_outs), _c_int_array(hw), L, num_anchors,
                          capi.ptr(anchors), capi.ptr(assigned), capi.ptr(pos_mask),
                          capi.ptr(neg_mask), capi.ptr(gt_cat),
                          _c_int_array(gt_offsets), N, _c_float_array(means), _c_float_array(stds),
                          float(beta), float(pos_weight), float(loss_weight_cls),
                          float(loss_weight_bbox), capi.ptr(lc), capi.ptr(lb), capi.ptr(nt),
                          capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_rpn_loss', rc)
    return lc, lb, nt


class _RpnLossFn(torch.autograd.Function):
    """Differentiable (w.r.t. the fused head outputs) form of the fused RPN loss."""

    @staticmethod
    def forward(ctx, cfg, anchors, assigned, pos_mask, neg_mask, gt_cat, *level_outs):
        outs = [o.detach() for o in level_outs]
        lc, lb, nt = _rpn_loss_launch(outs, cfg[0], anchors, assigned, pos_mask, neg_mask, gt_cat,
                                      *cfg[1:])
        ctx.cfg = cfg
        ctx.save_for_backward(anchors, assigned, pos_mask, neg_mask, gt_cat, nt, *outs)
        ctx.mark_non_differentiable(nt)
        return lc, lb, nt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lc, g_lb, _g_nt):
        anchors, assigned, pos_mask, neg_mask, gt_cat, nt = ctx.saved_tensors[:6]
        outs = list(ctx.saved_tensors[6:])
        (num_anchors, gt_offsets, means, stds, beta, pos_weight, w_cls, w_bbox) = ctx.cfg
        lib = capi.load()
        L = len(outs)
        N = outs[0].shape[0]
        hw = [int(o.shape[1] * o.shape[2]) for o in outs]
        douts = [torch.zeros_like(o) for o in outs]
        rc = lib.bgs_rpn_loss_grad(_c_ptr_array(outs), _c_ptr_array(douts), _c_int_array(hw), L,
                                   num_anchors, capi.ptr(anchors), capi.ptr(assigned),
                                   capi.ptr(pos_mask), capi.ptr(neg_mask), capi.ptr(gt_cat),
                                   _c_int_array(gt_offsets), N, _c_float_array(means),
                                   _c_float_array(stds), float(beta), float(pos_weight),
                                   float(w_cls), float(w_bbox), capi.ptr(nt),
                                   capi.ptr(_f32c(g_lc)), capi.ptr(_f32c(g_lb)),
                                   capi.current_stream(anchors.device))
        capi.check('bgs_rpn_loss_grad', rc)
        return (None,) * 6 + tuple(douts)


def rpn_loss(level_outs, num_anchors, anchors, assigned, pos_mask, neg_mask, gt_cat, gt_offsets,
             means, stds, beta, pos_weight=-1, loss_weight_cls=1.0, loss_weight_bbox=1.0):
    """Per-level RPN losses ``(loss_cls [L], loss_bbox [L], num_total_samples [1])`` from the
    fused head outputs ``[N,H,W,A+4A]`` of every level and the sampled-anchor masks.
    Differentiable w.r.t. ``level_outs`` when they require grad."""
    _require_cuda(anchors, assigned, pos_mask, neg_mask, gt_cat, *level_outs)
    pos_mask, neg_mask, gt_cat = pos_mask.contiguous(), neg_mask.contiguous(), _f32c(gt_cat)
    args = (num_anchors, tuple(int(o) for o in gt_offsets), tuple(means), tuple(stds), beta,
            pos_weight, loss_weight_cls, loss_weight_bbox)
    if torch.is_grad_enabled() and any(o.requires_grad for o in level_outs):
        return _RpnLossFn.apply(args, anchors, assigned, pos_mask, neg_mask, gt_cat, *level_outs)
    return _rpn_loss_launch(list(level_outs), num_anchors, anchors, assigned, pos_mask, neg_mask,
                            gt_cat, *args[1:])


_KEY_COUNTERS = {}


def _draw_counter(device, name):
    """Per (device, sampler) draw counter (device int64 ``[1]``), advanced with a tensor op per
    call.  One counter per sampler: the RPN sampler may run on a second stream next to the RoI
    sampler (detectors._rpn_forward_train), and a shared counter would be a cross-stream race."""
    key = (device.index, name)
    ctr = _KEY_COUNTERS.get(key)
    if ctr is None:
        ctr = torch.zeros(1, dtype=torch.int64, device=device)
        _KEY_COUNTERS[key] = ctr
    ctr.add_(1)
    return ctr


def random_keys(n, device):
    """``[n]`` int64 sampling keys in ``[0, 2^62)`` from the counter-based device RNG
    (``bgs_random_keys``).  A per-device draw counter is advanced with a tensor op per call, so
    the launch is hipGraph-replayable and still draws fresh keys every replay."""
    lib = capi.load()
    device = torch.device(device)
    ctr = _draw_counter(device, 'keys')
    out = torch.empty((n,), dtype=torch.int64, device=device)
    seed = (torch.initial_seed() * 0x9E3779B1 + 0x5851F42D) & 0xFFFFFFFFFFFFFFFF
    rc = lib.bgs_random_keys(seed, capi.ptr(ctr), int(n), capi.ptr(out),
                             capi.current_stream(device))
    capi.check('bgs_random_keys', rc)
    return out


def sample_pos_neg(assigned, num, pos_fraction, neg_pos_ub=-1):
    """RPN RandomSampler for a whole batch in one launch: ``assigned [N, A]`` int32 ->
    ``(pos_mask, neg_mask) [N, A]`` uint8 with the exact counts of base_sampler.py:56-73."""
    _require_cuda(assigned)
    lib = capi.load()
    assert assigned.dim() == 2 and assigned.dtype == torch.int32 and assigned.is_contiguous()
    N, A = assigned.shape
    dev = assigned.device
    ctr = _draw_counter(dev, 'pos_neg')
    pos = torch.empty((N, A), dtype=torch.uint8, device=dev)
    neg = torch.empty((N, A), dtype=torch.uint8, device=dev)
    seed = (torch.initial_seed() * 0x9E3779B1 + 0x2545F491) & 0xFFFFFFFFFFFFFFFF
    ws = _workspace(lib.bgs_sample_pos_neg_workspace_bytes(N), dev)
    rc = lib.bgs_sample_pos_neg(capi.ptr(assigned), N, A, int(num), float(pos_fraction),
                                float(neg_pos_ub), seed, capi.ptr(ctr), capi.ptr(pos), capi.ptr(neg),
                                capi.ptr(ws), capi.current_stream(dev))
    capi.check('bgs_sample_pos_neg', rc)
    return pos, neg


def sample_rois(assigned_list, num, pos_fraction, gt_counts=None):
    """RoI-head RandomSampler for a batch: per image ``assigned [A_n]`` int32 (candidates = GT
    boxes then proposals) -> ``inds [N, num]`` int64 (positives first), ``is_pos``, ``valid``
    ``[N, num]`` uint8.  One launch; ``A_n <= 4096``.  ``gt_counts`` (list of ints: the GT boxes in
    front of each image's candidates): also returns ``gt_ind [N, num]`` int32 (assigned gt index of
    every sampled row, -1 = none) and ``is_gt [N, num]`` uint8 from the same launch."""
    _require_cuda(*assigned_list)
    lib = capi.load()
    N = len(assigned_list)
    dev = assigned_list[0].device
    for a in assigned_list:
        assert a.dtype == torch.int32 and a.is_contiguous() and a.dim() == 1
    ctr = _draw_counter(dev, 'rois')
    inds = torch.empty((N, num), dtype=torch.int64, device=dev)
    is_pos = torch.empty((N, num), dtype=torch.uint8, device=dev)
    valid = torch.empty((N, num), dtype=torch.uint8, device=dev)
    seed = (torch.initial_seed() * 0x9E3779B1 + 0x68E31DA4) & 0xFFFFFFFFFFFFFFFF
    if gt_counts is not None:
        gt_ind = torch.empty((N, num), dtype=torch.int32, device=dev)
        is_gt = torch.empty((N, num), dtype=torch.uint8, device=dev)
        rc = lib.bgs_sample_rois_ex(_c_ptr_array(assigned_list),
                                    _c_int_array([int(a.numel()) for a in assigned_list]),
                                    _c_int_array([int(g) for g in gt_counts]), N, int(num),
                                    float(pos_fraction), seed, capi.ptr(ctr), capi.ptr(inds),
                                    capi.ptr(is_pos), capi.ptr(valid), capi.ptr(gt_ind), capi.ptr(is_gt),
                                    capi.current_stream(dev))
        capi.check('bgs_sample_rois_ex', rc)
        return inds, is_pos, valid, gt_ind, is_gt
    rc = lib.bgs_sample_rois(_c_ptr_array(assigned_list),
                             _c_int_array([int(a.numel()) for a in assigned_list]), N, int(num),
                             float(pos_fraction), seed, capi.ptr(ctr), capi.ptr(inds),
                             capi.ptr(is_pos), capi.ptr(valid), capi.current_stream(dev))
    capi.check('bgs_sample_rois', rc)
    return inds, is_pos, valid


def sample_rois_balanced(assigned_list, max_overlaps_list, num, pos_fraction, gt_counts, neg_pos_ub=-1,
                         pos_mode=1, neg_mode=1, floor_thr=-1, floor_fraction=0, num_bins=3, extra=False,
                         seed=None, draw_counter=None):
    """The balanced RoI samplers of Libra R-CNN for a batch in one launch (``bgs_sample_rois_balanced``): per image
    ``assigned [A_n]`` int32 and ``max_overlaps [A_n]`` float32 (candidates = ``gt_counts[n]`` GT boxes with overlap
    1.0, then the proposals; ``A_n <= 4096``) -> ``inds [N, num]`` int64 (positives first), ``is_pos``, ``valid``
    ``[N, num]`` uint8, and with ``extra`` also ``gt_ind`` int32 and ``is_gt`` uint8 as ``sample_rois`` returns them.

    ``pos_mode`` 0 = RandomSampler, 1 = InstanceBalancedPosSampler; ``neg_mode`` 0 = RandomSampler, 1 =
    IoUBalancedNegSampler with ``floor_thr`` / ``floor_fraction`` / ``num_bins``.  ``seed`` / ``draw_counter`` (device
    int64 ``[1]``): a caller's own draw instead of the per-device counter; the same pair returns the same bits."""
    _require_cuda(*assigned_list, *max_overlaps_list)
    lib = capi.load()
    N = len(assigned_list)
    assert len(max_overlaps_list) == N and len(gt_counts) == N
    dev = assigned_list[0].device
    for a, o in zip(assigned_list, max_overlaps_list):
        assert a.dtype == torch.int32 and a.is_contiguous() and a.dim() == 1
        assert o.dtype == torch.float32 and o.is_contiguous() and o.shape == a.shape
    ctr = _draw_counter(dev, 'rois_balanced') if draw_counter is None else draw_counter
    if seed is None:
        seed = (torch.initial_seed() * 0x9E3779B1 + 0x3C6EF372) & 0xFFFFFFFFFFFFFFFF
    inds = torch.empty((N, num), dtype=torch.int64, device=dev)
    is_pos = torch.empty((N, num), dtype=torch.uint8, device=dev)
    valid = torch.empty((N, num), dtype=torch.uint8, device=dev)
    args = (_c_ptr_array(assigned_list), _c_ptr_array(max_overlaps_list),
            _c_int_array([int(a.numel()) for a in assigned_list]), _c_int_array(gt_counts), N, int(num),
            float(pos_fraction), float(neg_pos_ub), int(pos_mode), int(neg_mode), float(floor_thr),
            float(floor_fraction), int(num_bins), int(seed), capi.ptr(ctr), capi.ptr(inds), capi.ptr(is_pos),
            capi.ptr(valid))
    if extra:
        gt_ind = torch.empty((N, num), dtype=torch.int32, device=dev)
        is_gt = torch.empty((N, num), dtype=torch.uint8, device=dev)
        rc = lib.bgs_sample_rois_balanced_ex(*args, capi.ptr(gt_ind), capi.ptr(is_gt), capi.current_stream(dev))
        capi.check('bgs_sample_rois_balanced_ex', rc)
        return inds, is_pos, valid, gt_ind, is_gt
    rc = lib.bgs_sample_rois_balanced(*args, capi.current_stream(dev))
    capi.check('bgs_sample_rois_balanced', rc)
    return inds, is_pos, valid


def decode_proposals(level_outs, level_counts, num_anchors, anchors, top_idx, top_logit, img_hw,
                     means, stds, wh_ratio_clip=16 / 1000):
    """``[N,L,nmax,5]`` decoded + clamped proposals (score = sigmoid of the top logit)."""
    _require_cuda(anchors, top_idx, top_logit, *level_outs)
    lib = capi.load()
    L = len(level_outs)
    N, L2, nmax = top_idx.shape
    assert L2 == L and top_idx.dtype == torch.int64 and top_idx.is_contiguous()
    assert top_logit.dtype == torch.float32 and top_logit.is_contiguous()
    hw = [int(o.shape[1] * o.shape[2]) for o in level_outs]
    out = torch.empty((N, L, nmax, 5), dtype=torch.float32, device=anchors.device)
    flat_hw = []
    for h, w in img_hw:
        flat_hw += [int(h), int(w)]
    rc = lib.bgs_decode_proposals(_c_ptr_array(level_outs), _c_int_array(hw),
                                  _c_int_array(level_counts), L, num_anchors, capi.ptr(anchors),
                                  capi.ptr(top_idx), capi.ptr(top_logit), N, _c_int_array(flat_hw),
                                  _c_float_array(means), _c_float_array(stds),
                                  float(wh_ratio_clip), nmax, capi.ptr(out),
                                  capi.current_stream(anchors.device))
    capi.check('bgs_decode_proposals', rc)
    return out


def refine_boxes(rois, labels, bbox_pred, img_shapes, means, stds, wh_ratio_clip=16 / 1000):
    """Cascade stage hand-over (``regress_by_class`` + ``delta2bbox`` for all images) in one launch:
    ``rois [K,5]`` (image index, box), ``labels [K]`` int64 (ignored when ``bbox_pred`` has 4 columns:
    class-agnostic), ``bbox_pred [K, 4 or 4*classes]``, ``img_shapes`` = per-image ``(h, w)`` clip bounds
    -> ``[K,4]`` boxes."""
    _require_cuda(rois, labels, bbox_pred)
    lib = capi.load()
    K, cols = bbox_pred.shape
    assert rois.dtype == torch.float32 and bbox_pred.dtype == torch.float32
    assert rois.is_contiguous() and bbox_pred.is_contiguous() and tuple(rois.shape) == (K, 5)
    lab = None
    if cols > 4:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == K
        lab = labels
    out = torch.empty((K, 4), dtype=torch.float32, device=rois.device)
    hw = [int(v) for s_ in img_shapes for v in s_[:2]]
    rc = lib.bgs_refine_boxes(capi.ptr(rois), capi.ptr(lab), capi.ptr(bbox_pred), K, cols,
                              _c_int_array(hw), len(img_shapes), _c_float_array(means),
                              _c_float_array(stds), float(wh_ratio_clip), capi.ptr(out),
                              capi.current_stream(rois.device))
    capi.check('bgs_refine_boxes', rc)
    return out


def rcnn_targets(boxes_list, assigned_list, inds_list, valid_list, gt_labels_list, gt_cat,
                 gt_offsets, num, means, stds, pos_weight=-1):
    """Sampled RoIs -> ``rois [N*num,5]``, ``labels`` i64, ``label_weights``, ``bbox_targets``,
    ``bbox_weights`` (positives first per image, as bbox_target_single lays them out)."""
    _require_cuda(gt_cat, *boxes_list)
    lib = capi.load()
    N = len(boxes_list)
    dev = gt_cat.device
    for b, a, i, g in zip(boxes_list, assigned_list, inds_list, gt_labels_list):
        assert b.dtype == torch.float32 and b.is_contiguous() and b.dim() == 2
        assert a.dtype == torch.int32 and a.is_contiguous()
        assert i.dtype == torch.int64 and i.is_contiguous() and i.numel() == num
        assert g.dtype == torch.int64 and g.is_contiguous()
    valid_u8 = [None if v is None else v.to(torch.uint8).contiguous() for v in valid_list]
    rois = torch.empty((N * num, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((N * num,), dtype=torch.int64, device=dev)
    lw = torch.empty((N * num,), dtype=torch.float32, device=dev)
    bt = torch.empty((N * num, 4), dtype=torch.float32, device=dev)
    bw = torch.empty((N * num, 4), dtype=torch.float32, device=dev)
    rc = lib.bgs_rcnn_targets(_c_ptr_array(boxes_list), _c_int_array([b.shape[1] for b in boxes_list]),
                              _c_ptr_array(assigned_list), _c_ptr_array(inds_list),
                              _c_ptr_array(valid_u8) if any(v is not None for v in valid_u8) else None,
                              _c_ptr_array(gt_labels_list), capi.ptr(_f32c(gt_cat)),
                              _c_int_array(gt_offsets), N, num, _c_float_array(means),
                              _c_float_array(stds), float(pos_weight), capi.ptr(rois),
                              capi.ptr(labels), capi.ptr(lw), capi.ptr(bt), capi.ptr(bw),
                              capi.current_stream(dev))
    capi.check('bgs_rcnn_targets', rc)
    return rois, labels, lw, bt, bw


def selftest_wave_reduce(values):
    """Runs the device self-test of the wave reduction primitive (64 floats in)."""
    _require_cuda(values)
    lib = capi.load()
    v = _f32c(values)
    assert v.numel() == 64
    out = torch.empty(4, dtype=torch.float32, device=v.device)
    capi.check('bgs_selftest_wave_reduce',
               lib.bgs_selftest_wave_reduce(capi.ptr(v), capi.ptr(out),
                                            capi.current_stream(v.device)))
    return out


# ----------------------------------------------------------------------------------------
# mask branch (csrc/mask_head.hip): targets, single-channel logits, fused BCE
# ----------------------------------------------------------------------------------------
def mask_target(gt_masks, rois, gt_inds, valid, mask_size):
    """``gt_masks``: per image a uint8 device tensor ``[G_n, H, W]``; ``rois [P, >=5]`` float
    (batch_ind, x1, y1, x2, y2); ``gt_inds [P]`` int32; ``valid [P]`` bool/uint8 or None ->
    ``[P, S, S]`` float targets (mask_target.py:16-38 incl. the cv2 INTER_LINEAR uint8 resize)."""
    import ctypes
    _require_cuda(rois, gt_inds, valid, *gt_masks)
    lib = capi.load()
    N = len(gt_masks)
    Hm, Wm = int(gt_masks[0].shape[1]), int(gt_masks[0].shape[2])
    for m in gt_masks:
        assert m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape[1:]) == (Hm, Wm)
    rois = _f32c(rois)
    P = rois.shape[0]
    gt_inds = gt_inds.to(torch.int32).contiguous()
    v8 = None if valid is None else valid.to(torch.uint8).contiguous()
    out = torch.empty((P, mask_size, mask_size), dtype=torch.float32, device=rois.device)
    ptrs = (ctypes.c_void_p * N)(*[m.data_ptr() if m.numel() else None for m in gt_masks])
    ng = (ctypes.c_int * N)(*[int(m.shape[0]) for m in gt_masks])
    rc = lib.bgs_mask_target(ptrs, ng, N, Hm, Wm, capi.ptr(rois), int(rois.shape[1]),
                             capi.ptr(gt_inds), capi.ptr(v8), P, int(mask_size), capi.ptr(out),
                             capi.current_stream(rois.device))
    capi.check('bgs_mask_target', rc)
    return out


def mask_paste(probs, boxes, scale_factor, thr, img_h, img_w):
    """``FCNMaskHead.get_seg_masks`` without the RLE step (fcn_mask_head.py:156-176) in one launch
    (``bgs_mask_paste_u8``): ``probs [K, S, S]`` float = sigmoid of each detection's own class channel,
    ``boxes [K, >=4]`` -> dense ``uint8 [K, img_h, img_w]``: the box (divided by ``scale_factor``, truncated to int as
    the reference does) receives ``cv2.resize(prob, (w, h), INTER_LINEAR) > thr``, everything else is 0."""
    _require_cuda(probs, boxes)
    lib = capi.load()
    probs, boxes = _f32c(probs), _f32c(boxes)
    K, S, S2 = probs.shape
    assert S == S2 and boxes.dim() == 2 and boxes.shape[0] == K and boxes.shape[1] >= 4
    out = torch.empty((K, int(img_h), int(img_w)), dtype=torch.uint8, device=probs.device)
    if K == 0:
        return out
    rc = lib.bgs_mask_paste_u8(capi.ptr(probs), capi.ptr(boxes), int(boxes.shape[1]), K, S, float(scale_factor),
                               float(thr), int(img_h), int(img_w), capi.ptr(out),
                               capi.current_stream(probs.device))
    capi.check('bgs_mask_paste_u8', rc)
    return out


def _per_detection(v, K, width, dtype):
    """A scalar / pair, or per-detection host values (sequence, numpy, tensor) -> numpy ``[K]`` or ``[K, width]``."""
    import numpy as np
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    a = np.asarray(v, dtype=dtype)
    shape = (K,) if width == 1 else (K, width)
    if a.shape == shape:
        return np.ascontiguousarray(a)
    if a.shape == shape[1:]:
        return np.ascontiguousarray(np.broadcast_to(a, shape))
    raise ValueError('expected shape %r or %r, got %r' % (shape[1:], shape, a.shape))


def mask_rle_counts(probs, boxes, scale_factor, thr, img_hw):
    """The device half of :func:`mask_rle`: -> ``(counts uint32 [total], offsets int64 [K + 1], sizes int32 [K, 2])`` as
    host numpy arrays; detection ``k``'s run lengths are ``counts[offsets[k] : offsets[k + 1]]``."""
    import numpy as np
    _require_cuda(probs, boxes)
    lib = capi.load()
    probs, boxes = _f32c(probs), _f32c(boxes)
    K, S, S2 = probs.shape
    assert S == S2 and boxes.dim() == 2 and boxes.shape[0] == K and boxes.shape[1] >= 4
    hw = _per_detection(img_hw, K, 2, np.int32)
    sf = _per_detection(scale_factor, K, 1, np.float32)
    if K == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64), hw
    if hw.min() <= 0 or not (sf > 0).all():
        raise ValueError('mask_rle: image sizes and scale factors must be positive')
    max_h, max_w = int(hw[:, 0].max()), int(hw[:, 1].max())
    dev = probs.device
    table = torch.from_numpy(np.concatenate([hw.reshape(-1), sf.view(np.int32)])).to(dev)      # one upload
    hw_d, sf_d = table[:2 * K], table[2 * K:].view(torch.float32)
    ws_bytes = int(lib.bgs_mask_rle_workspace_bytes(K, max_w))
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=dev)
    runs = torch.empty(K, dtype=torch.int32, device=dev)
    stream = capi.current_stream(dev)
    geom = (capi.ptr(probs), capi.ptr(boxes), int(boxes.shape[1]), K, S, capi.ptr(hw_d), capi.ptr(sf_d), float(thr),
            max_h, max_w, capi.ptr(ws), ws_bytes)
    capi.check('bgs_mask_rle_count', lib.bgs_mask_rle_count(*geom, capi.ptr(runs), stream))
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(runs, 0, dtype=torch.int64)
    offsets_h = offsets.cpu().numpy()                      # the one synchronisation: the size of the result
    total = int(offsets_h[-1])
    positions = torch.empty(total, dtype=torch.int32, device=dev)
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    capi.check('bgs_mask_rle_write', lib.bgs_mask_rle_write(*geom, capi.ptr(offsets), total, capi.ptr(positions),
                                                            capi.ptr(counts), stream))
    return counts.cpu().numpy().view(np.uint32), offsets_h, hw


def mask_rle(probs, boxes, scale_factor, thr, img_hw):
    """``FCNMaskHead.get_seg_masks`` INCLUDING the RLE step (fcn_mask_head.py:156-181) without the dense tensor
    (``bgs_mask_rle_count`` / ``bgs_mask_rle_write`` + the host string codec): ``probs [K, S, S]``, ``boxes [K, >=4]``
    as in :func:`mask_paste`; ``scale_factor`` a float or ``[K]``, ``img_hw`` ``(h, w)`` or ``[K, 2]`` (host values:
    a list, numpy or a CPU tensor — per detection, so that the detections of several images go through one call).
    Returns a list of ``K`` dicts ``{'size': [h, w], 'counts': bytes}``, the type ``pycocotools.mask.encode(m)[0]``
    returns; ``rle.decode`` of entry ``k`` equals ``mask_paste(...)[k]``."""
    from . import rle
    counts, offsets, hw = mask_rle_counts(probs, boxes, scale_factor, thr, img_hw)
    strings = rle.pack_strings(counts, offsets)
    sizes = hw.tolist()
    return [{'size': sizes[k], 'counts': strings[k]} for k in range(len(strings))]


# ----------------------------------------------------------------------------------------
# polygons -> COCO RLE, RLE merge  (pycocotools maskApi.c rleFrPoly / rleMerge; csrc/poly_rle.hip)
# ----------------------------------------------------------------------------------------
POLY_COORD_LIMIT = 1e6
RLE_MAX_AREA = 2 ** 31 - 1
_RLE_PARITY, _RLE_UNION, _RLE_INTERSECT = 0, 1, 2


def _poly_tables(objects, sizes):
    """The host checks and the flat tables of :func:`poly_rle_counts`: ``(xy float64 [2 V], part_off int64 [P + 1],
    obj_off int64 [O + 1], hw int32 [O, 2])``."""
    import numpy as np
    objects = list(objects)
    O = len(objects)
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2) if O else np.zeros((0, 2), np.int64)
    if hw.shape[0] == 1 and O > 1:
        hw = np.broadcast_to(hw, (O, 2))
    if hw.shape[0] != O:
        raise ValueError('poly_rle: %d objects but %d sizes' % (O, hw.shape[0]))
    if O and hw.min() <= 0:
        raise ValueError('poly_rle: image sizes must be positive')
    if O and (hw[:, 0] * hw[:, 1]).max() > RLE_MAX_AREA:
        raise ValueError('poly_rle: h * w must not exceed 2^31 - 1 (column-major positions are 32 bit)')
    parts = []
    nparts = np.zeros(O, np.int64)
    for o, obj in enumerate(objects):
        if not isinstance(obj, (list, tuple)) or (len(obj) and not hasattr(obj[0], '__len__')):
            raise ValueError('poly_rle: object %d is not a list of parts (flat coordinate lists)' % o)
        nparts[o] = len(obj)
        parts.extend(obj)
    lens = np.fromiter((len(p) for p in parts), dtype=np.int64, count=len(parts))
    if lens.size and (lens.min() == 0 or (lens & 1).any()):
        raise ValueError('poly_rle: a part needs a non-empty, even number of coordinates (x0, y0, x1, y1, ...)')
    xy = np.fromiter(itertools.chain.from_iterable(parts), dtype=np.float64, count=int(lens.sum()))
    if xy.size and not (np.isfinite(xy).all() and np.abs(xy).max() <= POLY_COORD_LIMIT):
        raise ValueError('poly_rle: coordinates must be finite and within +-%g' % POLY_COORD_LIMIT)
    part_off = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens // 2, out=part_off[1:])
    obj_off = np.zeros(O + 1, np.int64)
    np.cumsum(nparts, out=obj_off[1:])
    return xy, part_off, obj_off, np.ascontiguousarray(hw, dtype=np.int32)


def _rle_device(device, what):
    if not torch.cuda.is_available():
        raise RuntimeError('%s runs only on the GPU (hand-written HIP kernels); there is no CPU fallback' % what)
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda':
        raise RuntimeError('%s runs only on the GPU (hand-written HIP kernels); got device %s' % (what, dev))
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def _scan0(x):
    """int tensor ``[n]`` -> its exclusive scan, int64 ``[n + 1]``."""
    out = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=x.device)
    out[1:] = torch.cumsum(x, 0, dtype=torch.int64)
    return out


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rle_finish(lib, S, bound, dev, runs, write):
    """``runs`` int32 ``[S]`` on the device -> the host pair ``(counts uint32 [total], offsets int64 [S + 1])``:
    the offsets and the counts share one device buffer (``bound`` >= total) and come back in ONE copy."""
    import numpy as np
    head = 2 * (S + 1)
    out = torch.empty(head + bound, dtype=torch.int32, device=dev)
    out_off = out[:head].view(torch.int64)
    out_off[:1].zero_()
    out_off[1:] = torch.cumsum(runs, 0, dtype=torch.int64)
    write(out_off, out[head:])
    host = out.cpu().numpy()
    offsets = host[:head].view(np.int64).copy()
    total = int(offsets[-1])
    return host[head:head + total].view(np.uint32).copy(), offsets


def poly_rle_counts(objects, sizes, device=None):
    """Polygons -> COCO run lengths on the device (``rleFrPoly`` of every part, then ``rleMerge`` of an object's
    parts: what ``pycocotools.mask.frPyObjects`` + ``merge`` give; csrc/poly_rle.hip).  ``objects``: a list of ``O``
    objects, each a list of parts, each a flat ``[x0, y0, x1, y1, ...]``; ``sizes``: ``(h, w)`` or ``[O, 2]``.
    Returns the host triple of :func:`mask_rle_counts`: ``(counts uint32 [total], offsets int64 [O + 1], sizes int32
    [O, 2])``.  Seven launches whatever ``O`` is, one host read (the number of boundary crossings, which sizes the
    buffers) and one copy back; bitwise the same on every call."""
    return poly_rle_counts_from_tables(*_poly_tables(objects, sizes), device=device)


def poly_rle_counts_from_tables(xy, part_off, obj_off, hw, device=None):
    """:func:`poly_rle_counts` on the flat host tables (``_poly_tables``: ``xy`` float64 ``[2 V]``, ``part_off`` int64
    ``[P + 1]`` in vertices, ``obj_off`` int64 ``[O + 1]`` in parts, ``hw`` int32 ``[O, 2]``, already checked)."""
    import numpy as np
    O, P, V = hw.shape[0], part_off.size - 1, xy.size // 2
    if O == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64), hw
    dev = _rle_device(device, 'poly_rle')
    if P == 0:                                             # only empty masks
        return ((hw[:, 0].astype(np.int64) * hw[:, 1]).astype(np.uint32), np.arange(O + 1, dtype=np.int64), hw)
    lib = capi.load()
    with torch.cuda.device(dev):
        stream = capi.current_stream(dev)
        table = torch.from_numpy(np.concatenate([part_off, obj_off, hw.reshape(-1).view(np.int64),
                                                 xy.view(np.int64)])).to(dev)          # one upload
        part_off_d, obj_off_d = table[:P + 1], table[P + 1:P + O + 2]
        hw_d = table[P + O + 2:P + 2 * O + 2].view(torch.int32)
        xy_d = table[P + 2 * O + 2:].view(torch.float64)
        edge_pts = torch.empty(V, dtype=torch.int64, device=dev)
        capi.check('bgs_poly_rle_edge_points',
                   lib.bgs_poly_rle_edge_points(capi.ptr(xy_d), capi.ptr(part_off_d), _np_ptr(part_off), V, P,
                                                capi.ptr(edge_pts), stream))
        pt_off = _scan0(edge_pts)
        geom = (capi.ptr(xy_d), capi.ptr(part_off_d), capi.ptr(obj_off_d), capi.ptr(hw_d), V, P, O, capi.ptr(pt_off))
        tally = torch.zeros(P, dtype=torch.int32, device=dev)
        capi.check('bgs_poly_rle_crossings', lib.bgs_poly_rle_crossings(*geom, None, 0, capi.ptr(tally), None, stream))
        cross_off = _scan0(tally)
        C = int(cross_off[-1].item())                      # the one synchronisation: sizes every buffer below
        if C > RLE_MAX_AREA:
            raise ValueError('poly_rle: %d boundary crossings in one call; split the batch' % C)
        keys = torch.empty(max(C, 1), dtype=torch.int32, device=dev)
        trans = torch.empty(max(C, 1), dtype=torch.int32, device=dev)
        events = torch.empty(max(C, 1), dtype=torch.int32, device=dev)
        cursor = torch.zeros(P, dtype=torch.int32, device=dev)
        capi.check('bgs_poly_rle_crossings',
                   lib.bgs_poly_rle_crossings(*geom, capi.ptr(cross_off), C, capi.ptr(cursor), capi.ptr(keys), stream))
        tcnt = torch.empty(P, dtype=torch.int32, device=dev)
        capi.check('bgs_poly_rle_resolve',
                   lib.bgs_poly_rle_resolve(capi.ptr(keys), capi.ptr(cross_off), None, P, _RLE_PARITY, None, None,
                                            capi.ptr(hw_d), capi.ptr(obj_off_d), O, C, capi.ptr(trans),
                                            capi.ptr(tcnt), None, stream))
        ev_off = _scan0(tcnt)
        capi.check('bgs_poly_rle_events_from_transitions',
                   lib.bgs_poly_rle_events_from_transitions(capi.ptr(trans), capi.ptr(cross_off), capi.ptr(tcnt),
                                                            capi.ptr(ev_off), P, C, capi.ptr(events), stream))
        merged, mcnt = keys, torch.empty(O, dtype=torch.int32, device=dev)      # (the keys are spent: reuse)
        runs = torch.empty(O, dtype=torch.int32, device=dev)
        capi.check('bgs_poly_rle_resolve',
                   lib.bgs_poly_rle_resolve(capi.ptr(events), capi.ptr(ev_off), capi.ptr(obj_off_d), O, _RLE_UNION,
                                            capi.ptr(obj_off_d), None, capi.ptr(hw_d), None, 0, C, capi.ptr(merged),
                                            capi.ptr(mcnt), capi.ptr(runs), stream))

        def write(out_off, out):
            capi.check('bgs_poly_rle_write',
                       lib.bgs_poly_rle_write(capi.ptr(merged), capi.ptr(ev_off), capi.ptr(obj_off_d), capi.ptr(mcnt),
                                              O, capi.ptr(obj_off_d), None, None, capi.ptr(hw_d), C,
                                              capi.ptr(out_off), C + O, capi.ptr(out), stream))
        counts, offsets = _rle_finish(lib, O, C + O, dev, runs, write)
    return counts, offsets, hw


def poly_rle(objects, sizes, device=None):
    """:func:`poly_rle_counts` as RLE dicts: a list of ``O`` ``{'size': [h, w], 'counts': bytes}``, what
    ``mask.merge(mask.frPyObjects(parts, h, w))`` returns for every object."""
    from . import rle
    counts, offsets, hw = poly_rle_counts(objects, sizes, device)
    strings = rle.pack_strings(counts, offsets)
    sz = hw.tolist()
    return [{'size': sz[k], 'counts': strings[k]} for k in range(len(strings))]


def rle_merge_counts(counts, list_off, grp_off, sizes, intersect=False, device=None):
    """``rleMerge`` for ``G`` groups of run lists at once (stage B of csrc/poly_rle.hip): list ``l`` owns
    ``counts[list_off[l] : list_off[l + 1]]`` (uint32, host), group ``g`` owns lists ``grp_off[g] .. grp_off[g + 1]``
    (at least one), ``sizes`` ``[G, 2]`` (h, w).  Returns ``(counts uint32, offsets int64 [G + 1])`` on the host: the
    canonical run list of every union (intersection); a group of one list comes back unchanged.  Three launches, no
    host read before the copy back."""
    import numpy as np
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    list_off = np.ascontiguousarray(list_off, dtype=np.int64).reshape(-1)
    grp_off = np.ascontiguousarray(grp_off, dtype=np.int64).reshape(-1)
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1, 2))
    G, L, R = grp_off.size - 1, list_off.size - 1, counts.size
    if G < 0 or L < 0 or hw.shape[0] != G:
        raise ValueError('rle_merge: offsets must be [n + 1] and sizes [G, 2]')
    if G == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64)
    if grp_off[0] != 0 or grp_off[-1] != L or (np.diff(grp_off) <= 0).any():
        raise ValueError('rle_merge: every group needs at least one mask')
    if list_off[0] != 0 or list_off[-1] != R or (np.diff(list_off) <= 0).any():
        raise ValueError('rle_merge: an RLE without runs')
    area = hw[:, 0] * hw[:, 1]
    if hw.min() <= 0 or area.max() > RLE_MAX_AREA:
        raise ValueError('rle_merge: sizes must be positive with h * w <= 2^31 - 1')
    sums = np.add.reduceat(counts.astype(np.int64), list_off[:-1])
    if (sums != np.repeat(area, np.diff(grp_off))).any():
        raise ValueError('rle_merge: the runs of a mask do not cover h * w pixels')
    dev = _rle_device(device, 'rle_merge')
    lib = capi.load()
    ev_base = list_off[grp_off] - grp_off
    E = R - L
    with torch.cuda.device(dev):
        stream = capi.current_stream(dev)
        table = torch.from_numpy(np.concatenate([list_off, grp_off, ev_base,
                                                 hw.astype(np.int32).reshape(-1).view(np.int64)])).to(dev)
        list_off_d, grp_off_d = table[:L + 1], table[L + 1:L + G + 2]
        ev_base_d = table[L + G + 2:L + 2 * G + 3]
        hw_d = table[L + 2 * G + 3:].view(torch.int32)
        counts_d = torch.from_numpy(counts.view(np.int32)).to(dev)
        cum = torch.cumsum(counts_d, 0, dtype=torch.int64)
        events = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        trans = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        capi.check('bgs_poly_rle_events_from_runs',
                   lib.bgs_poly_rle_events_from_runs(capi.ptr(cum), capi.ptr(list_off_d), _np_ptr(list_off), L, R,
                                                     capi.ptr(events), stream))
        tcnt = torch.empty(G, dtype=torch.int32, device=dev)
        runs = torch.empty(G, dtype=torch.int32, device=dev)
        mode = _RLE_INTERSECT if intersect else _RLE_UNION
        capi.check('bgs_poly_rle_resolve',
                   lib.bgs_poly_rle_resolve(capi.ptr(events), capi.ptr(ev_base_d), None, G, mode, capi.ptr(grp_off_d),
                                            capi.ptr(list_off_d), capi.ptr(hw_d), None, 0, E, capi.ptr(trans),
                                            capi.ptr(tcnt), capi.ptr(runs), stream))

        def write(out_off, out):
            capi.check('bgs_poly_rle_write',
                       lib.bgs_poly_rle_write(capi.ptr(trans), capi.ptr(ev_base_d), None, capi.ptr(tcnt), G,
                                              capi.ptr(grp_off_d), capi.ptr(list_off_d), capi.ptr(counts_d),
                                              capi.ptr(hw_d), E, capi.ptr(out_off), R + G, capi.ptr(out), stream))
        return _rle_finish(lib, G, R + G, dev, runs, write)


def rle_merge(groups, intersect=False, device=None):
    """``pycocotools.mask.merge`` for many groups at once: ``groups`` is a list of lists of RLE dicts (``counts`` a
    compressed ``bytes`` / ``str`` or a list of ints); returns one ``{'size', 'counts': bytes}`` per group.  Masks of
    different sizes in one group are a ``ValueError``."""
    import numpy as np
    from . import rle
    from .lvis_eval import _rle_tables
    groups = [list(g) for g in groups]
    if not groups:
        return []
    if any(len(g) == 0 for g in groups):
        raise ValueError('rle_merge: every group needs at least one mask')
    flat = [r for g in groups for r in g]
    if any(not isinstance(r, dict) for r in flat):
        raise ValueError('rle_merge: the masks are RLE dicts (polygons go through poly_rle)')
    counts, list_off, sz = _rle_tables(flat, 'rle_merge')
    grp_off = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=grp_off[1:])
    first = sz[grp_off[:-1]]
    if (sz != np.repeat(first, np.diff(grp_off), axis=0)).any():
        raise ValueError('rle_merge: masks of different sizes in one group')
    out, off = rle_merge_counts(counts, list_off, grp_off, first, intersect, device)
    strings = rle.pack_strings(out, off)
    sizes = first.tolist()
    return [{'size': sizes[g], 'counts': strings[g]} for g in range(len(strings))]


# ----------------------------------------------------------------------------------------
# LVIS evaluation  (lvis-api/lvis/eval.py:116-292; csrc/lvis_eval.hip)
# ----------------------------------------------------------------------------------------
class LvisProblems(object):
    """The CSR description of the (image, category) problems of an evaluation, validated once on the host and uploaded
    once: ``dt_off`` / ``gt_off`` / ``iou_off`` int64 ``[P + 1]`` as host numpy (``.dt_off`` ...) and as device tensors
    (``.dt_off_d`` ...); ``P``, ``ND``, ``NG`` and ``total`` (the number of IoU entries)."""

    def __init__(self, dt_off, gt_off, device):
        import numpy as np
        dt_off = np.ascontiguousarray(dt_off, dtype=np.int64).reshape(-1)
        gt_off = np.ascontiguousarray(gt_off, dtype=np.int64).reshape(-1)
        if dt_off.shape != gt_off.shape or dt_off.size < 1:
            raise ValueError('lvis problems: dt_off and gt_off must both be [P + 1]')
        for o in (dt_off, gt_off):
            if o[0] != 0 or (np.diff(o) < 0).any():
                raise ValueError('lvis problems: offsets must start at 0 and never decrease')
        self.P = int(dt_off.size) - 1
        self.ND, self.NG = int(dt_off[-1]), int(gt_off[-1])
        self.dt_off, self.gt_off = dt_off, gt_off
        self.iou_off = np.zeros(self.P + 1, dtype=np.int64)
        np.cumsum(np.diff(dt_off) * np.diff(gt_off), out=self.iou_off[1:])
        self.total = int(self.iou_off[-1])
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('balancedgroupsoftmax_amd ops run only on the GPU (hand-written HIP kernels); '
                               'got device %s. There is no CPU fallback.' % self.device)
        table = torch.from_numpy(np.stack([dt_off, gt_off, self.iou_off])).to(self.device)      # one upload
        self.dt_off_d, self.gt_off_d, self.iou_off_d = table[0], table[1], table[2]


def _f64c(t, shape_tail, n, what):
    t = t.detach().to(torch.float64).contiguous()
    if tuple(t.shape) != (n,) + shape_tail:
        raise ValueError('%s: expected shape %r, got %r' % (what, (n,) + shape_tail, tuple(t.shape)))
    return t


def lvis_box_iou(dt_boxes, gt_boxes, problems):
    """``mask_utils.iou(dt, gt, iscrowd=0)`` of ``LVISEval.compute_iou`` (eval.py:168-192) over ``[x, y, w, h]`` boxes
    for every problem in one launch (``bgs_lvis_box_iou``): ``dt_boxes [ND, 4]`` (score order inside a problem),
    ``gt_boxes [NG, 4]``, ``problems`` a :class:`LvisProblems` -> fp64 ``[total]``: problem ``p``'s row-major
    ``[D_p, G_p]`` matrix begins at ``problems.iou_off[p]``.  fp64, one rounding per operation, as ``bbIou``."""
    _require_cuda(dt_boxes, gt_boxes)
    lib = capi.load()
    pr = problems
    dt = _f64c(dt_boxes, (4,), pr.ND, 'lvis_box_iou dt_boxes')
    gt = _f64c(gt_boxes, (4,), pr.NG, 'lvis_box_iou gt_boxes')
    out = torch.empty(pr.total, dtype=torch.float64, device=pr.device)
    rc = lib.bgs_lvis_box_iou(capi.ptr(dt), capi.ptr(gt), capi.ptr(pr.dt_off_d), capi.ptr(pr.gt_off_d),
                              capi.ptr(pr.iou_off_d), pr.P, pr.ND, pr.NG, pr.total, capi.ptr(out),
                              capi.current_stream(pr.device))
    capi.check('bgs_lvis_box_iou', rc)
    return out


def _rle_table(counts, offsets, sizes, n, what):
    import numpy as np
    if torch.is_tensor(counts):
        _require_cuda(counts)
        raise TypeError('%s: run lengths are host arrays (what mask_rle_counts returns)' % what)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1, 2)
    if offsets.size != n + 1 or sizes.shape[0] != n:
        raise ValueError('%s: expected %d masks, got offsets %r and sizes %r' % (what, n, offsets.shape, sizes.shape))
    if offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] > counts.size:
        raise ValueError('%s: offsets must start at 0, never decrease and end inside the counts' % what)
    return counts, offsets, sizes


def lvis_rle_iou(dt_rles, gt_rles, problems):
    """The same matrices for masks given as run lengths (``rleIou`` with ``iscrowd = 0``; ``bgs_lvis_rle_iou``).
    ``dt_rles`` / ``gt_rles``: ``(counts uint32 [total], offsets int64 [K + 1], sizes [K, 2])`` host arrays, the triple
    :func:`mask_rle_counts` returns.  Both masks of a pair must have the same size (checked here, per problem).
    One lane walks the two run lists of a pair in step; no dense mask is built."""
    import numpy as np
    lib = capi.load()
    pr = problems
    dc, do, ds = _rle_table(*dt_rles, pr.ND, 'lvis_rle_iou dt_rles')
    gc, go, gs = _rle_table(*gt_rles, pr.NG, 'lvis_rle_iou gt_rles')
    nd, ng = np.diff(pr.dt_off), np.diff(pr.gt_off)
    both = np.nonzero((nd > 0) & (ng > 0))[0]
    if both.size:
        # every mask of a problem against the size of the problem's first ground truth
        ref = np.zeros((pr.P, 2), np.int64)
        ref[both] = gs[pr.gt_off[both]]
        has = np.zeros(pr.P, bool)
        has[both] = True
        for sizes, n in ((ds, nd), (gs, ng)):
            owner = np.repeat(np.arange(pr.P), n)
            bad = has[owner] & (sizes != ref[owner]).any(axis=1)
            if bad.any():
                raise ValueError('lvis_rle_iou: masks of different sizes in problem %d' % int(owner[np.argmax(bad)]))
    dev = pr.device
    dc_d = torch.from_numpy(dc.view(np.int32)).to(dev)
    gc_d = torch.from_numpy(gc.view(np.int32)).to(dev)
    do_d, go_d = torch.from_numpy(do).to(dev), torch.from_numpy(go).to(dev)
    out = torch.empty(pr.total, dtype=torch.float64, device=dev)
    rc = lib.bgs_lvis_rle_iou(capi.ptr(dc_d), capi.ptr(do_d), capi.ptr(gc_d), capi.ptr(go_d), capi.ptr(pr.dt_off_d),
                              capi.ptr(pr.gt_off_d), capi.ptr(pr.iou_off_d), pr.P, pr.ND, pr.NG, pr.total,
                              capi.ptr(out), capi.current_stream(dev))
    capi.check('bgs_lvis_rle_iou', rc)
    return out


def lvis_match(ious, problems, dt_area, gt_area, gt_ignore, not_exhaustive, area_rng, iou_thrs, tables=True):
    """The greedy matching of ``LVISEval.evaluate_img`` (eval.py:194-292) for every problem, area range and threshold
    in one launch (``bgs_lvis_match``).  ``ious`` fp64 ``[total]`` (:func:`lvis_box_iou` / :func:`lvis_rle_iou`),
    ``dt_area [ND]`` / ``gt_area [NG]`` fp64, ``gt_ignore [NG]`` and ``not_exhaustive [P]`` bool / uint8 device
    tensors; ``area_rng`` ``[A, 2]`` and ``iou_thrs`` ``[T]`` host float64 values (A <= 4, T <= 16).
    Returns ``(dt_match int32 [ND, A, T], dt_ignore uint8 [ND, A, T], dt_bits int32 [A, ND], gt_ignore uint8
    [A, NG])``: ``dt_match`` is the ground truth's index inside its problem or -1; ``dt_bits`` packs bit ``t`` =
    matched and bit ``16 + t`` = ignored.  ``tables=False`` skips the two full tables (they are None)."""
    import numpy as np
    _require_cuda(ious, dt_area, gt_area, gt_ignore, not_exhaustive)
    lib = capi.load()
    pr = problems
    dev = pr.device
    rng = np.ascontiguousarray(area_rng, dtype=np.float64).reshape(-1, 2)
    thr = np.ascontiguousarray(iou_thrs, dtype=np.float64).reshape(-1)
    A, T = int(rng.shape[0]), int(thr.shape[0])
    ious = _f64c(ious, (), pr.total, 'lvis_match ious')
    dt_area = _f64c(dt_area, (), pr.ND, 'lvis_match dt_area')
    gt_area = _f64c(gt_area, (), pr.NG, 'lvis_match gt_area')
    gt_ignore = gt_ignore.to(torch.uint8).contiguous()
    nel = not_exhaustive.to(torch.uint8).contiguous()
    if gt_ignore.numel() != pr.NG or nel.numel() != pr.P:
        raise ValueError('lvis_match: gt_ignore must be [NG] and not_exhaustive [P]')
    dt_match = torch.empty((pr.ND, A, T), dtype=torch.int32, device=dev) if tables else None
    dt_ig = torch.empty((pr.ND, A, T), dtype=torch.uint8, device=dev) if tables else None
    dt_bits = torch.empty((A, pr.ND), dtype=torch.int32, device=dev)
    gt_ig = torch.empty((A, pr.NG), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.bgs_lvis_match_workspace_bytes(pr.NG, A, T))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    rc = lib.bgs_lvis_match(capi.ptr(ious), capi.ptr(pr.dt_off_d), capi.ptr(pr.gt_off_d), capi.ptr(pr.iou_off_d),
                            pr.P, pr.ND, pr.NG, capi.ptr(dt_area), capi.ptr(gt_area), capi.ptr(gt_ignore),
                            capi.ptr(nel), rng.ctypes.data_as(ctypes.c_void_p), A,
                            thr.ctypes.data_as(ctypes.c_void_p), T, capi.ptr(ws), ws_bytes, capi.ptr(dt_match),
                            capi.ptr(dt_ig), capi.ptr(dt_bits), capi.ptr(gt_ig), capi.current_stream(dev))
    capi.check('bgs_lvis_match', rc)
    return dt_match, dt_ig, dt_bits, gt_ig


def lvis_accumulate(dt_bits, gt_ignore, dt_score, cat_dt_off, cat_gt_off, rec_thrs, T):
    """``LVISEval.accumulate`` (eval.py:294-422) for every category, area range and threshold in one launch
    (``bgs_lvis_accumulate``).  ``dt_bits`` int32 ``[A, ND]`` and ``gt_ignore`` uint8 / bool ``[A, NG]`` device
    tensors as :func:`lvis_match` returns them, ``dt_score`` fp64 ``[ND]`` device tensor; ``cat_dt_off`` /
    ``cat_gt_off`` int64 ``[K + 1]``: category ``k`` owns detections ``cat_dt_off[k]:cat_dt_off[k + 1]`` and ground
    truths ``cat_gt_off[k]:cat_gt_off[k + 1]`` (host arrays are checked here and uploaded; device tensors are taken
    as they are, the kernel skips a category whose offsets leave the buffers); ``rec_thrs`` ``[R]`` host float64
    values; ``T`` the number of threshold bits in use (A <= 4, T <= 16, R <= 256).
    Returns device tensors ``(precision fp64 [T, R, K, A], recall fp64 [T, K, A])``, every element written.

    The order of a category's detections (descending score, equal scores in the order given) is NOT computed by a
    kernel of this package: it is the runtime's sort, two stable ``torch.sort`` calls (the negated scores ascending,
    then the category index).  The counting and the fp64 arithmetic are ``bgs_lvis_accumulate``."""
    import numpy as np
    _require_cuda(dt_bits, gt_ignore, dt_score)
    thr = np.ascontiguousarray(rec_thrs, dtype=np.float64).reshape(-1)
    R, T = int(thr.shape[0]), int(T)
    if dt_bits.dim() != 2 or gt_ignore.dim() != 2 or gt_ignore.shape[0] != dt_bits.shape[0]:
        raise ValueError('lvis_accumulate: dt_bits must be [A, ND] and gt_ignore [A, NG]')
    if dt_bits.dtype != torch.int32:
        raise ValueError('lvis_accumulate: dt_bits must be int32 (the packed bits of lvis_match)')
    A, ND, NG = int(dt_bits.shape[0]), int(dt_bits.shape[1]), int(gt_ignore.shape[1])
    if tuple(dt_score.shape) != (ND,):
        raise ValueError('lvis_accumulate: dt_score must be [ND] = [%d], got %r' % (ND, tuple(dt_score.shape)))
    if A < 1 or T < 1 or R < 1:
        raise ValueError('lvis_accumulate: A, T and the number of recall thresholds must be positive')
    dev = dt_bits.device
    offs = []
    for o, n, what in ((cat_dt_off, ND, 'cat_dt_off'), (cat_gt_off, NG, 'cat_gt_off')):
        if torch.is_tensor(o):
            _require_cuda(o)
            if o.dtype != torch.int64 or o.dim() != 1 or o.numel() < 1:
                raise ValueError('lvis_accumulate: %s must be int64 [K + 1]' % what)
            offs.append(o.contiguous())
        else:
            o = np.ascontiguousarray(o, dtype=np.int64).reshape(-1)
            if o.size < 1 or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != n:
                raise ValueError('lvis_accumulate: %s must start at 0, never decrease and end at %d' % (what, n))
            offs.append(o)
    if offs[0].shape[0] != offs[1].shape[0]:
        raise ValueError('lvis_accumulate: cat_dt_off and cat_gt_off must both be [K + 1]')
    K = int(offs[0].shape[0]) - 1
    lib = capi.load()
    # the entry's own limits, asked before any device work: with no category it validates and launches nothing
    capi.check('bgs_lvis_accumulate', lib.bgs_lvis_accumulate(None, None, None, None, None, 0, 0, 0, A, T,
                                                              thr.ctypes.data_as(ctypes.c_void_p), R, None, None, None))
    with torch.cuda.device(dev):
        if not torch.is_tensor(offs[0]) and not torch.is_tensor(offs[1]):
            both = torch.from_numpy(np.stack(offs)).to(dev)                                # one upload
            dt_off_d, gt_off_d = both[0], both[1]
        else:
            dt_off_d, gt_off_d = [o if torch.is_tensor(o) else torch.from_numpy(o).to(dev) for o in offs]
        dt_bits = dt_bits.detach().contiguous()
        gt_ignore = gt_ignore.detach().to(torch.uint8).contiguous()
        score = dt_score.detach().to(torch.float64).contiguous()
        by_score = torch.sort(-score, stable=True)[1]
        cat = torch.searchsorted(dt_off_d[1:].contiguous(), by_score, right=True)         # the category of each
        order = by_score[torch.sort(cat, stable=True)[1]].contiguous()
        precision = torch.empty((T, R, K, A), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A), dtype=torch.float64, device=dev)
        rc = lib.bgs_lvis_accumulate(capi.ptr(dt_bits), capi.ptr(gt_ignore), capi.ptr(order), capi.ptr(dt_off_d),
                                     capi.ptr(gt_off_d), K, ND, NG, A, T, thr.ctypes.data_as(ctypes.c_void_p), R,
                                     capi.ptr(precision), capi.ptr(recall), capi.current_stream(dev))
    capi.check('bgs_lvis_accumulate', rc)
    return precision, recall


# ----------------------------------------------------------------------------------------
# Proposal recall  (mmdet/core/evaluation/recall.py:7-37, bbox_overlaps.py:4-49; csrc/recall_match.hip)
# ----------------------------------------------------------------------------------------
RECALL_MAX_K, RECALL_MAX_T = 8, 16
RECALL_MAX_G, RECALL_MAX_N = 2048, 4096


def _recall_boxes(t, what):
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError('recall_match: %s must be [n, 4] (x1, y1, x2, y2), got %r' % (what, tuple(t.shape)))
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t       # (the kernel loads a box as one 16-byte word)


def _recall_check_boxes(b, what):
    """finite, x2 - x1 + 1 > 0 and a finite positive float32 area, on the device: one host read"""
    if b.shape[0]:
        w, h = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
        area = w * h
        if not bool((torch.isfinite(b).all(dim=1) & torch.isfinite(area) & (area > 0) & (w > 0)).all()):
            raise ValueError('recall_match: %s must be finite boxes of positive area' % what)


def _recall_table(a, dtype, what):
    import numpy as np
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError('recall_match: %s must be a 1-d integer table' % what)
    return np.ascontiguousarray(a, dtype=dtype)


def recall_match(gt_boxes, gt_off, prob_img, prop_boxes, prop_off, proposal_nums, iou_thrs, check=True):
    """``bbox_overlaps`` + the greedy assignment of ``_recalls`` (recall.py:16-29) + its threshold counts (recall.py:35)
    for every problem and every proposal count in one launch (``bgs_recall_match``).

    ``gt_boxes [NG, 4]`` / ``prop_boxes [NP, 4]``: float32 device tensors ``(x1, y1, x2, y2)``, the proposals already
    in evaluation order inside each image.  ``gt_off [P + 1]``, ``prob_img [P]``, ``prop_off [n_img + 1]``: integer
    tables (numpy arrays or lists; a tensor is copied to the host, they are validated there): problem ``p`` owns ground
    truths ``gt_off[p]:gt_off[p + 1]`` and reads the proposals ``prop_off[i]:prop_off[i + 1]`` of image ``i =
    prob_img[p]``.  ``proposal_nums [K]`` ascending ints (K <= 8), ``iou_thrs [T]`` float64 values (T <= 16).
    At most 2048 ground truths per problem and ``min(proposals of an image, proposal_nums[-1]) <= 4096``.
    Boxes must be finite with positive area (``ValueError``): the reference divides by zero or carries NaN there;
    ``check=False`` is for a caller that has made that check itself (``recall.py`` on its host arrays).  A box is loaded
    as one 16-byte word: a tensor whose data does not begin on a 16-byte boundary is copied first.

    Returns device tensors ``(gt_ious float32 [K, NG], counts int32 [P, K, T])``: ``gt_ious[k, gt_off[p] + j]`` is the
    IoU of the j-th pick of problem ``p`` (-1 once the proposals ran out, 0 with no proposal at all),
    ``counts[p, k, t]`` the number of its picks with ``float64(iou) >= iou_thrs[t]``."""
    import numpy as np
    gt = _recall_boxes(gt_boxes, 'gt_boxes')
    pr = _recall_boxes(prop_boxes, 'prop_boxes')
    if pr.device != gt.device:
        raise ValueError('recall_match: gt_boxes and prop_boxes must be on one device')
    gt_off = _recall_table(gt_off, np.int64, 'gt_off')
    prob_img = _recall_table(prob_img, np.int32, 'prob_img')
    prop_off = _recall_table(prop_off, np.int64, 'prop_off')
    nums = np.asarray(proposal_nums)
    if nums.ndim != 1 or nums.size < 1 or not np.issubdtype(nums.dtype, np.integer):
        raise ValueError('recall_match: proposal_nums must be a non-empty 1-d integer array')
    thr = np.ascontiguousarray(iou_thrs, dtype=np.float64).reshape(-1)
    K, T = int(nums.size), int(thr.size)
    if K > RECALL_MAX_K:
        raise ValueError('recall_match: at most %d proposal_nums, got %d' % (RECALL_MAX_K, K))
    if T < 1 or T > RECALL_MAX_T:
        raise ValueError('recall_match: between 1 and %d iou_thrs, got %d' % (RECALL_MAX_T, T))
    if (nums < 0).any() or (np.diff(nums) < 0).any() or nums.max() > 0x7fffffff:
        raise ValueError('recall_match: proposal_nums must be non-negative and ascending, got %r' % (nums.tolist(),))
    nums = np.ascontiguousarray(nums, dtype=np.int32)
    NG, NP = int(gt.shape[0]), int(pr.shape[0])
    for o, n, what in ((gt_off, NG, 'gt_off'), (prop_off, NP, 'prop_off')):
        if o.size < 1 or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != n:
            raise ValueError('recall_match: %s must start at 0, never decrease and end at %d' % (what, n))
    P, n_img = int(gt_off.size) - 1, int(prop_off.size) - 1
    if prob_img.size != P:
        raise ValueError('recall_match: prob_img must be [P] = [%d], got %r' % (P, prob_img.shape))
    if P and (prob_img.min() < 0 or prob_img.max() >= n_img):
        raise ValueError('recall_match: prob_img must lie in [0, %d)' % n_img)
    max_g = int(np.diff(gt_off).max()) if P else 0
    max_n = int(min(np.diff(prop_off)[prob_img].max(), nums[-1])) if P else 0
    if max_g > RECALL_MAX_G:
        raise ValueError('recall_match: a problem holds %d ground truths, the limit is %d' % (max_g, RECALL_MAX_G))
    if max_n > RECALL_MAX_N:
        raise ValueError('recall_match: %d proposals of one image are in use, the limit is %d (lower proposal_nums)'
                         % (max_n, RECALL_MAX_N))
    _require_cuda(gt, pr)                  # (the tables above are host work: their refusals need no device)
    dev = gt.device
    with torch.cuda.device(dev):
        if check:
            _recall_check_boxes(gt, 'gt_boxes')
            _recall_check_boxes(pr, 'prop_boxes')
        gt_ious = torch.zeros((K, NG), dtype=torch.float32, device=dev)
        counts = torch.zeros((P, K, T), dtype=torch.int32, device=dev)
        if P == 0:
            return gt_ious, counts
        # one upload: the int64 offsets and (as int64) the image of each problem
        table = torch.from_numpy(np.concatenate([gt_off, prop_off, prob_img.astype(np.int64)])).to(dev)
        gt_off_d, prop_off_d = table[:P + 1], table[P + 1:P + n_img + 2]
        prob_img_d = table[P + n_img + 2:].to(torch.int32)
        lib = capi.load()
        rc = lib.bgs_recall_match(capi.ptr(gt), capi.ptr(gt_off_d), capi.ptr(prob_img_d), capi.ptr(pr),
                                  capi.ptr(prop_off_d), nums.ctypes.data_as(ctypes.c_void_p), K,
                                  thr.ctypes.data_as(ctypes.c_void_p), T, P, n_img, NG, NP, max_g, max_n,
                                  capi.ptr(gt_ious), capi.ptr(counts), capi.current_stream(dev))
    capi.check('bgs_recall_match', rc)
    return gt_ious, counts


def mask_gt_logits(feat, weight, bias, labels):
    """``feat [P, pixels, C]``, ``weight [K, C]``, ``labels [P]`` -> ``[P, pixels]`` logits of each
    RoI's own class channel (no gradient: test-time / inspection path)."""
    _require_cuda(feat, weight, bias, labels)
    lib = capi.load()
    feat, weight = _f32c(feat), _f32c(weight)
    P, pix, C = feat.shape
    out = torch.empty((P, pix), dtype=torch.float32, device=feat.device)
    rc = lib.bgs_mask_gt_logits(capi.ptr(feat), capi.ptr(weight),
                                capi.ptr(None if bias is None else _f32c(bias)),
                                capi.ptr(labels.to(torch.int64).contiguous()), P, pix, C,
                                weight.shape[0], capi.ptr(out), capi.current_stream(feat.device))
    capi.check('bgs_mask_gt_logits', rc)
    return out


class _MaskBceFn(torch.autograd.Function):
    """loss[1] = mean over (valid RoIs x pixels) of BCE(<feat, W[label]> + b[label], target);
    gradients for feat, W, b come from the same launch (scaled by the upstream scalar after)."""

    @staticmethod
    def forward(ctx, feat, weight, bias, labels, target, valid):
        lib = capi.load()
        f, w = _f32c(feat), _f32c(weight)
        b = None if bias is None else _f32c(bias)
        P, pix, C = f.shape
        dev = f.device
        lab = labels.to(torch.int64).contiguous()
        tgt = _f32c(target)
        v8 = None if valid is None else valid.to(torch.uint8).contiguous()
        nvalid = torch.full((), float(P), device=dev) if v8 is None else v8.sum().float()
        norm = (1.0 / (nvalid.clamp(min=1.0) * pix)).reshape(1).contiguous()
        need = [feat.requires_grad, weight.requires_grad, bias is not None and bias.requires_grad]
        dfeat = torch.empty_like(f) if need[0] else None
        dw = torch.zeros_like(w) if (need[1] or need[2]) else None
        db = torch.zeros(w.shape[0], dtype=torch.float32, device=dev) if dw is not None else None
        part = torch.empty((lib.bgs_mask_bce_partials(P),), dtype=torch.float32, device=dev)
        rc = lib.bgs_mask_bce(capi.ptr(f), capi.ptr(w), capi.ptr(b), capi.ptr(lab), capi.ptr(tgt),
                              capi.ptr(v8), capi.ptr(norm), P, pix, C, w.shape[0], capi.ptr(part),
                              capi.ptr(dfeat), capi.ptr(dw), capi.ptr(db),
                              capi.current_stream(dev))
        capi.check('bgs_mask_bce', rc)
        ctx.grads = (dfeat, dw, db if bias is not None else None)
        return (part.sum() * norm[0]).reshape(1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dfeat, dw, db = ctx.grads
        s = g.reshape(())
        return (None if dfeat is None else dfeat * s, None if dw is None else dw * s,
                None if db is None else db * s, None, None, None)


def mask_bce(feat, weight, bias, labels, target, valid=None):
    """Fused single-channel ``conv_logits`` + ``mask_cross_entropy`` -> loss ``[1]``."""
    _require_cuda(feat, weight, bias, labels, target, valid)
    assert feat.dim() == 3 and weight.dim() == 2 and feat.shape[2] == weight.shape[1]
    return _MaskBceFn.apply(feat, weight, bias, labels, target, valid)


# ----------------------------------------------------------------------------------------
# Mask Scoring R-CNN branch (csrc/mask_iou.hip): targets, the head's input, the GT-channel logits with
# their gradient, the gathered MSE loss
# ----------------------------------------------------------------------------------------
def _refuse_dtype(name, t, *dtypes):
    if t.dtype not in dtypes:
        raise TypeError('%s: dtype %s (expected %s)' % (name, t.dtype, ' or '.join(str(d) for d in dtypes)))


def mask_iou_target(gt_masks, rois, gt_inds, valid, z, mask_targets, mask_thr_binary):
    """``MaskIoUHead.get_target`` (maskiou_head.py:102-175) in two launches on bitmaps resident in HBM
    (``bgs_mask_iou_target``): ``gt_masks`` / ``rois [P, >=5]`` / ``gt_inds [P]`` / ``valid [P]`` as :func:`mask_target`,
    ``z [P, S, S]`` each RoI's own-class mask LOGITS, ``mask_targets [P, S, S]`` -> ``[P]`` float, 0 in invalid slots.
    No host read."""
    import ctypes
    _require_cuda(rois, gt_inds, valid, z, mask_targets, *gt_masks)
    N = len(gt_masks)
    if N == 0:
        raise ValueError('mask_iou_target: gt_masks is empty (per image a uint8 [G, H, W] tensor)')
    Hm, Wm = int(gt_masks[0].shape[1]), int(gt_masks[0].shape[2])
    for m in gt_masks:
        _refuse_dtype('mask_iou_target: gt_masks', m, torch.uint8)
        if m.dim() != 3 or tuple(m.shape[1:]) != (Hm, Wm) or not m.is_contiguous():
            raise ValueError('mask_iou_target: gt_masks are contiguous [G, %d, %d] bitmaps, got %s'
                             % (Hm, Wm, tuple(m.shape)))
    _refuse_dtype('mask_iou_target: z', z, torch.float32)
    _refuse_dtype('mask_iou_target: mask_targets', mask_targets, torch.float32)
    _refuse_dtype('mask_iou_target: rois', rois, torch.float32)
    P = int(rois.shape[0])
    if rois.dim() != 2 or rois.shape[1] < 5 or z.dim() != 3 or z.shape[1] != z.shape[2] or \
            tuple(z.shape) != tuple(mask_targets.shape) or z.shape[0] != P or gt_inds.numel() != P or \
            (valid is not None and valid.numel() != P):
        raise ValueError('mask_iou_target: rois [P, >=5], gt_inds [P], valid [P], z and mask_targets [P, S, S]; got '
                         '%s %s %s %s %s' % (tuple(rois.shape), tuple(gt_inds.shape),
                                             None if valid is None else tuple(valid.shape), tuple(z.shape),
                                             tuple(mask_targets.shape)))
    lib = capi.load()
    rois, z, mt = _f32c(rois), _f32c(z), _f32c(mask_targets)
    gt_inds = gt_inds.to(torch.int32).contiguous()
    v8 = None if valid is None else valid.to(torch.uint8).contiguous()
    out = torch.empty((P,), dtype=torch.float32, device=rois.device)
    total = sum(int(m.shape[0]) for m in gt_masks)
    areas = torch.empty((max(total, 1),), dtype=torch.int64, device=rois.device)
    ptrs = (ctypes.c_void_p * N)(*[m.data_ptr() if m.numel() else None for m in gt_masks])
    ng = (ctypes.c_int * N)(*[int(m.shape[0]) for m in gt_masks])
    rc = lib.bgs_mask_iou_target(ptrs, ng, N, Hm, Wm, capi.ptr(rois), int(rois.shape[1]), capi.ptr(gt_inds),
                                 capi.ptr(v8), capi.ptr(z), capi.ptr(mt), P, int(z.shape[1]), float(mask_thr_binary),
                                 capi.ptr(areas), capi.ptr(out), capi.current_stream(rois.device))
    capi.check('bgs_mask_iou_target', rc)
    return out


class _MaskIouInputFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feat, z):
        lib = capi.load()
        f, zz = _f32c(feat), _f32c(z)
        P, h, w, C = f.shape
        out = torch.empty((P, h, w, C + 4), dtype=torch.float32, device=f.device)
        rc = lib.bgs_mask_iou_input_fwd(capi.ptr(f), capi.ptr(zz), P, h, w, C, capi.ptr(out),
                                        capi.current_stream(f.device))
        capi.check('bgs_mask_iou_input_fwd', rc)
        ctx.save_for_backward(zz)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx):
        zz, = ctx.saved_tensors
        lib = capi.load()
        dx = _f32c(dx)
        P, h, w, Cp = dx.shape
        dfeat = torch.empty((P, h, w, Cp - 4), dtype=torch.float32, device=dx.device) \
            if ctx.needs_input_grad[0] else None
        dz = torch.empty_like(zz) if ctx.needs_input_grad[1] else None
        rc = lib.bgs_mask_iou_input_bwd(capi.ptr(dx), capi.ptr(zz), P, h, w, Cp - 4, capi.ptr(dfeat), capi.ptr(dz),
                                        capi.current_stream(dx.device))
        capi.check('bgs_mask_iou_input_bwd', rc)
        return dfeat, dz


def mask_iou_input(feat, z):
    """The input of ``MaskIoUHead``'s first conv (maskiou_head.py:78-81) in one launch each way: ``feat [P, h, w, C]``
    NHWC mask RoI features, ``z [P, 2h, 2w]`` mask logits -> ``[P, h, w, C + 4]``: the features, ``max_pool2x2(sigmoid(z))``
    in channel ``C``, zeros above (the conv kernels need ``Cin % 4 == 0``)."""
    _require_cuda(feat, z)
    _refuse_dtype('mask_iou_input: feat', feat, torch.float32)
    _refuse_dtype('mask_iou_input: z', z, torch.float32)
    if feat.dim() != 4 or z.dim() != 3 or tuple(z.shape) != (feat.shape[0], 2 * feat.shape[1], 2 * feat.shape[2]):
        raise ValueError('mask_iou_input: feat [P, h, w, C] and z [P, 2h, 2w], got %s and %s'
                         % (tuple(feat.shape), tuple(z.shape)))
    if feat.shape[3] % 4 != 0:
        raise NotImplementedError('mask_iou_input: C % 4 != 0 (C = {})'.format(feat.shape[3]))
    return _MaskIouInputFn.apply(feat, z)


class _MaskGtLogitsFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feat, weight, bias, labels):
        lab = labels.to(torch.int64).contiguous()
        ctx.save_for_backward(feat, weight, lab)
        ctx.has_bias = bias is not None
        return mask_gt_logits(feat, weight, bias, lab)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        feat, weight, lab = ctx.saved_tensors
        lib = capi.load()
        f, w, dz = _f32c(feat), _f32c(weight), _f32c(dz)
        P, pix, C = f.shape
        need = ctx.needs_input_grad
        dfeat = torch.empty_like(f) if need[0] else None
        dw = torch.zeros_like(w) if need[1] else None
        db = torch.zeros((w.shape[0],), dtype=torch.float32, device=f.device) if ctx.has_bias and need[2] else None
        rc = lib.bgs_mask_gt_logits_bwd(capi.ptr(dz), capi.ptr(f), capi.ptr(w), capi.ptr(lab), P, pix, C, w.shape[0],
                                        capi.ptr(dfeat), capi.ptr(dw), capi.ptr(db), capi.current_stream(f.device))
        capi.check('bgs_mask_gt_logits_bwd', rc)
        return dfeat, dw, db, None


def mask_gt_logits_autograd(feat, weight, bias, labels):
    """:func:`mask_gt_logits` with its gradient (``bgs_mask_gt_logits_bwd``): the reference feeds
    ``mask_pred[range, pos_labels]`` to the MaskIoU head undetached (mask_scoring_rcnn.py:153-154).  Rows of
    ``weight.grad`` / ``bias.grad`` shared by several RoIs are accumulated with fp32 atomics (as ``mask_bce``)."""
    _require_cuda(feat, weight, bias, labels)
    _refuse_dtype('mask_gt_logits_autograd: feat', feat, torch.float32)
    _refuse_dtype('mask_gt_logits_autograd: weight', weight, torch.float32)
    if feat.dim() != 3 or weight.dim() != 2 or feat.shape[2] != weight.shape[1] or labels.numel() != feat.shape[0]:
        raise ValueError('mask_gt_logits_autograd: feat [P, pixels, C], weight [K, C], labels [P]; got %s %s %s'
                         % (tuple(feat.shape), tuple(weight.shape), tuple(labels.shape)))
    if feat.shape[2] % 4 != 0 or feat.shape[2] > 1024:
        raise NotImplementedError('mask_gt_logits_autograd: C % 4 != 0 or C > 1024 (C = {})'.format(feat.shape[2]))
    return _MaskGtLogitsFn.apply(feat, weight, bias, labels)


class _MaskIouMseFn(torch.autograd.Function):
    """loss[1] = loss_weight * mean over the kept rows of (pred[p, label_p] - target_p)^2; the dense gradient comes
    from the same launch (scaled by the upstream scalar after)."""

    @staticmethod
    def forward(ctx, pred, labels, targets, valid, loss_weight, positive_only=True):
        lib = capi.load()
        pr, tg = _f32c(pred), _f32c(targets)
        P, K = pr.shape
        lab = None if labels is None else labels.to(torch.int64).contiguous()
        v8 = None if valid is None else valid.to(torch.uint8).contiguous()
        out = torch.empty((1,), dtype=torch.float32, device=pr.device)
        grad = torch.empty_like(pr) if ctx.needs_input_grad[0] else None
        rc = lib.bgs_mask_iou_mse_fwd_bwd(capi.ptr(pr), capi.ptr(lab), capi.ptr(tg), capi.ptr(v8), P, K,
                                          int(bool(positive_only)), float(loss_weight), capi.ptr(out), None, capi.ptr(grad),
                                          capi.current_stream(pr.device))
        capi.check('bgs_mask_iou_mse_fwd_bwd', rc)
        ctx.grad = grad
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return (None if ctx.grad is None else ctx.grad * g.reshape(()), None, None, None, None, None)


def mask_iou_mse_loss(pred, targets, labels=None, valid=None, loss_weight=1.0, positive_only=True):
    """``MaskIoUHead.loss`` + ``MSELoss`` (maskiou_head.py:92-99, mse_loss.py) in one launch: ``pred [P, K]`` with
    ``labels [P]`` (the column of each row) or the already gathered ``pred [P]`` without; rows with ``valid`` and
    ``target > 0`` are kept (NaN is not ``> 0``; ``positive_only=False``, the plain ``MSELoss``, keeps every valid
    row) -> ``loss_weight * mean (pred - target)^2`` as ``[1]``, 0 with a zero gradient when no row is kept.  Fixed
    summation order; the count stays on the device."""
    _require_cuda(pred, targets, labels, valid)
    _refuse_dtype('mask_iou_mse_loss: pred', pred, torch.float32)
    _refuse_dtype('mask_iou_mse_loss: targets', targets, torch.float32)
    if labels is None:
        if pred.dim() != 1:
            raise ValueError('mask_iou_mse_loss: without labels pred is the gathered [P], got %s' % (tuple(pred.shape),))
        pred = pred.reshape(-1, 1)
    else:
        _refuse_dtype('mask_iou_mse_loss: labels', labels, torch.int64, torch.int32)
    P = pred.shape[0]
    if pred.dim() != 2 or targets.dim() != 1 or targets.numel() != P or \
            (labels is not None and labels.numel() != P) or (valid is not None and valid.numel() != P):
        raise ValueError('mask_iou_mse_loss: pred [P, K], targets / labels / valid [P]; got %s %s %s %s'
                         % (tuple(pred.shape), tuple(targets.shape), None if labels is None else tuple(labels.shape),
                            None if valid is None else tuple(valid.shape)))
    return _MaskIouMseFn.apply(pred, labels, targets, valid, float(loss_weight), bool(positive_only))
