"""MI355X-native ContinuousTransformer — drop-in mirror of
stable_audio_tools/models/transformer.py (LayerNorm :215, RotaryEmbedding :92, GLU :252,
FeedForward :277, Attention :328, TransformerBlock :582, ContinuousTransformer :715): same class
names, constructor kwargs and state_dict keys (gamma/beta, to_qkv / to_q / to_kv / to_out,
ff.ff.0.proj / ff.ff.2, to_scale_shift_gate, project_in/out, rotary_pos_emb.inv_freq,
global_cond_embedder).

Execution: LayerNorm(+adaLN modulate), partial rotary, attention (self and GQA cross), SwiGLU and the
gate/residual epilogue are HIP kernels (csrc/dit_ops.hip, csrc/attention.hip); every projection is
linear.Linear on the native MFMA GEMM (csrc/gemm.hip) with the head split / rotary / SwiGLU / gate /
residual work of the block fused into the GEMM epilogues — no library GEMM.  Attention(qk_norm="ln" | "l2")
(attn_kwargs: {"qk_norm": ...}; the per-head q / k normalisation before the rotary, transformer.py:374-376,
:485-489) runs inside the same projection epilogue in bf16 inference (sat_gemm_qkv_norm_bf16) and on the
sat_qk_norm_fwd / sat_qk_norm_bwd kernels in training and fp32.  ContinuousTransformer(sliding_window=[left, right])
(flash-attn's window_size on every layer's self-attention, transformer.py:436, :845) runs on the windowed forward
kernel (sat_attention_fwd_window) in inference, fp32 and bf16, head dims 64 and 128; training with a window, a
window on cross-attention and a window over an fp8 input projection raise NotImplementedError.
TransformerBlock(layer_scale=True) (LayerScale :243, x = x + scale * branch(...), :684-712) is inference-only: the scale is folded into
the rows of each branch's output projection (a derived weight, cached per version of weight and scale), so it costs no launch;
TransformerBlock(add_rope=True) (:656, :672-673) gives the block a rotary table of its own, forward and backward.  These two, head dim
128, qk_norm "ln" and the window are the block of the transformer autoencoder (autoencoders.TAAEBlock).  The options of the reference
that no supported config enables raise NotImplementedError (qk_norm="dyt", differential attention, conformer, memory tokens, causal,
flex-attention masks, abs/sinusoidal position embeddings).

Forward AND backward run on the HIP kernels: every fused operator is a torch.autograd.Function whose
backward calls the matching kernel (LayerNorm+adaLN, rotary transpose, attention dQ / dK,dV with
probabilities recomputed from the saved log-sum-exp, SwiGLU, gate/residual); the projections' data and
weight gradients run on the same native GEMM (linear.LinearFn.backward).  Per-layer activation checkpointing
of the reference (transformer.py:28-30, :840-845) is optional here: off by default (288 GB of HBM), on with
`use_checkpointing=True` / `ContinuousTransformer.checkpointing = True` when the batch does not fit.
"""

import torch
from torch import nn

from . import _caches
from . import functional as _fn
from . import linear as _linear
from .linear import Linear, _lowp

# LayerNorm -> fp8 rows for an fp8 consumer (round 4); False (set by an A/B script): normalise to bf16, then quantise
fp8_ln_fused = True


def _ops():
    return _fn._ops(None)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, scale, shift, eps, g32=None, b32=None):
        """g32 / b32: optional fp32 copies of gamma / beta prepared by the caller (the kernels read fp32 parameters)."""
        ops = _ops()
        x = x.contiguous()
        if g32 is None:
            g32 = gamma.float().contiguous()
        if b32 is None and beta is not None:
            b32 = beta.float().contiguous()
        if any(ctx.needs_input_grad):   # (torch.is_grad_enabled() is always False inside Function.forward)
            y, mean, rstd = ops.layernorm(x, g32, b32, scale, shift, eps, save_stats=True)
            ctx.save_for_backward(x, g32, b32, scale, mean, rstd)
            ctx.ops = ops
            ctx.gdtype = gamma.dtype
        else:
            y = ops.layernorm(x, g32, b32, scale, shift, eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g32, b32, scale, mean, rstd = ctx.saved_tensors
        dx, dgamma, dscale, dshift = ctx.ops.layernorm_bwd(dy.contiguous(), x, g32, b32, scale, mean, rstd)
        if dscale is not None:
            dscale, dshift = dscale.to(scale.dtype), dshift.to(scale.dtype)
        return dx, dgamma.to(ctx.gdtype), None, dscale, dshift, None, None, None


class LayerNormResFn(torch.autograd.Function):
    """(LayerNorm(x), x) for a pre-norm residual branch x = x + f(LN(x)) (transformer.py:703-712): the second output is x itself, to be
    handed to the branch's output projection as `res`.  Autograd then delivers BOTH gradients of x to this node — through the normalised
    branch and along the residual path — and the LayerNorm backward kernel adds the latter in its own pass (sat_layernorm_bwd_res) instead
    of autograd launching an elementwise add of two (B, N, D) tensors per norm (round 6)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, g32, b32):
        ops = _ops()
        x = x.contiguous()
        y, mean, rstd = ops.layernorm(x, g32, b32, None, None, eps, save_stats=True)
        ctx.save_for_backward(x, g32, b32, mean, rstd)
        ctx.ops, ctx.gdtype = ops, gamma.dtype
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, g32, b32, mean, rstd = ctx.saved_tensors
        if dy is None:
            return dres, None, None, None, None, None
        if dres is not None and dres.dtype != dy.dtype:
            dres = dres.to(dy.dtype)
        dx, dgamma, _, _ = ctx.ops.layernorm_bwd(dy.contiguous(), x, g32, b32, None, mean, rstd,
                                                 dres=dres.contiguous() if dres is not None else None)
        return dx, dgamma.to(ctx.gdtype), None, None, None, None


class LayerNorm(nn.Module):
    def __init__(self, dim, bias=False, fix_scale=False, force_fp32=False, eps=1e-5):
        super().__init__()
        if fix_scale:
            self.register_buffer("gamma", torch.ones(dim))
        else:
            self.gamma = nn.Parameter(torch.ones(dim))
        if bias:
            # the backward kernel does not produce d(beta); no Stable Audio config sets norm_kwargs.bias
            raise NotImplementedError("LayerNorm(bias=True) is not on the HIP path (the reference default is a zero buffer)")
        else:
            self.register_buffer("beta", torch.zeros(dim))
        self.eps = eps
        self.force_fp32 = force_fp32   # statistics are always fp32 in the HIP kernel
        self._f32_cache = {}

    def _as_f32(self, name):
        """fp32 view of a parameter for the kernels; for a bf16/fp16 module the converted copy is cached until the
        parameter changes (in-place version counter / storage)."""
        t = getattr(self, name)
        if t.dtype == torch.float32:
            return t.detach()
        if not _caches.trackable(t):
            return t.detach().float().contiguous()
        key = (t.data_ptr(), _caches.version_of(t), t.device, _caches.epoch_of(t))
        hit = self._f32_cache.get(name)
        if hit is None or hit[0] != key:
            hit = (key, t.detach().float().contiguous())
            self._f32_cache[name] = hit
        return hit[1]

    def forward(self, x, scale=None, shift=None, fp8_for=None):
        """scale/shift: optional (B, D) adaLN modulation fused into the same pass: LN(x)*(1+scale)+shift.
        fp8_for: the ONE projection that consumes the result.  In inference, when that Linear runs in fp8 with per-row activation scales, the
        normalised rows leave the kernel as fp8 + row scales (linear.Fp8Rows): no bf16 LayerNorm output, no quantisation pass."""
        if (fp8_for is not None and fp8_for.fp8 and _linear.fp8_row_scales and not torch.is_grad_enabled() and x.dim() == 3
                and x.dtype == torch.bfloat16 and fp8_for.in_features % 16 == 0 and fp8_for.out_features % 8 == 0
                and fp8_for.fp8_weight() is not None and fp8_ln_fused):
            out = _ops().layernorm_fp8(x.contiguous(), self._as_f32("gamma"), self._as_f32("beta"), scale, shift, self.eps)
            if out is not None:
                return _linear.Fp8Rows(out[0], out[1], x.shape)
        return LayerNormFn.apply(x, self.gamma, self.beta, scale, shift, self.eps, self._as_f32("gamma"), self._as_f32("beta"))

    def with_residual(self, x):
        """(LN(x), x) — see LayerNormResFn; training path of the un-modulated pre-norm branches."""
        return LayerNormResFn.apply(x, self.gamma, self.beta, self.eps, self._as_f32("gamma"), self._as_f32("beta"))


class RotaryEmbedding(nn.Module):
    def __init__(self, dim, use_xpos=False, scale_base=512, interpolation_factor=1., base=10000, base_rescale_factor=1.):
        super().__init__()
        if use_xpos:
            raise NotImplementedError("use_xpos is dead code in the reference (transformer.py:143) and not implemented")
        base *= base_rescale_factor ** (dim / (dim - 2))
        inv_freq = 1. / (base ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq)
        assert interpolation_factor >= 1.
        self.interpolation_factor = interpolation_factor
        self.register_buffer("scale", None)

    def tables(self, seq_len):
        """(seq_len, dim/2, 2) fp32 cos/sin table (csrc/dit_ops.hip sat_rope_tables)."""
        inv = self.inv_freq.float().contiguous()
        if self.interpolation_factor != 1.:
            inv = inv / self.interpolation_factor
        return _ops().rope_tables(inv, seq_len)

    def forward_from_seq_len(self, seq_len):
        return self.tables(seq_len), 1.


class _RopeQKFn(torch.autograd.Function):
    """In-place rotary on the q and k slices of a fused (B, N, 3*H*dh) projection."""

    @staticmethod
    def forward(ctx, qkv, cs, heads, dh):
        ops = _ops()
        b, n, _ = qkv.shape
        hd = heads * dh
        ops.rope_apply_(qkv[..., 0:hd].unflatten(-1, (heads, dh)), cs)
        ops.rope_apply_(qkv[..., hd:2 * hd].unflatten(-1, (heads, dh)), cs)
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(cs)
        ctx.meta = (heads, dh, ops)
        return qkv

    @staticmethod
    def backward(ctx, g):
        (cs,) = ctx.saved_tensors
        heads, dh, ops = ctx.meta
        g = g.clone()
        hd = heads * dh
        ops.rope_apply_(g[..., 0:hd].unflatten(-1, (heads, dh)), cs, transpose=True)
        ops.rope_apply_(g[..., hd:2 * hd].unflatten(-1, (heads, dh)), cs, transpose=True)
        return g, None, None, None


class _AttentionCoreFn(torch.autograd.Function):
    """o = softmax(q k^T * scale) v  on csrc/attention.hip; backward = sat_attention_bwd (dQ and dK/dV kernels
    that recompute the probabilities from the saved log-sum-exp — nothing N x N is ever stored)."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        ops = _ops()
        if any(ctx.needs_input_grad[:3]):
            o, lse, planes = ops.attention(q, k, v, scale, return_planes=True)
            ctx.ops, ctx.scale, ctx.planes = ops, scale, planes
            ctx.shapes = (q.shape, k.shape)
            ctx.save_for_backward(o, lse)
            return o
        return ops.attention(q, k, v, scale)

    @staticmethod
    def backward(ctx, g):
        o, lse = ctx.saved_tensors
        (_, _, _, _), (_, hkv, nk, _) = ctx.shapes
        dq, dk, dv = ctx.ops.attention_bwd(ctx.planes, o, g.contiguous(), lse, ctx.scale, hkv, nk)
        return dq, dk, dv, None


class _SelfAttnFn(torch.autograd.Function):
    """The training path of a fused-projection self-attention as ONE autograd node (round 6): in-place rotary on the q / k thirds of
    the (B, N, 3*H*dh) projection, head split, attention core (transformer.py:155-174, :389-441 of the reference).  As separate nodes
    (_RopeQKFn, three slices, three permutes, _AttentionCoreFn) autograd rebuilt the projection's gradient from dq / dk / dv with three
    zero-filled (B, N, 3*H*dh) tensors, three strided copies into their thirds, two adds and a clone for the in-place rotary — nine
    activation-sized launches per layer; here dq / dk / dv leave the backward kernels as one (3, B, H, N, dh) buffer that ONE strided
    copy turns into the projection's layout, and the inverse rotary runs in place on that copy.
    `qkv` is rotated in place: it is the output of the projection GEMM, which nothing else reads (autograd raises if something saved it).
    With qk_norm (norm = (mode, fp32 tables), qn = the q_norm / k_norm parameters the gradients go to) the normalised + rotated q / k
    heads go to a buffer of their own (sat_qk_norm_fwd) and the raw projection is kept: the backward recomputes x-hat from it — never
    from the output and gamma, which may be zero — in the one pass that also undoes the rotary (sat_qk_norm_bwd, in place on dqkv)."""

    @staticmethod
    def forward(ctx, qkv, cs, heads, dh, scale, norm=None, *qn):
        ops = _ops()
        b, n, _ = qkv.shape
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        ctx.norm = norm
        if norm is not None:
            mode, tabs = norm
            need = any(ctx.needs_input_grad)
            qk = torch.empty(b, n, 2 * heads * dh, dtype=qkv.dtype, device=qkv.device)
            res = ops.qk_norm(qkv, 2 * heads, heads, mode, tabs, cs, out=qk, save_stats=need)
            qk5 = qk.view(b, n, 2, heads, dh)
            q, k = qk5[:, :, 0].permute(0, 2, 1, 3), qk5[:, :, 1].permute(0, 2, 1, 3)
            v = qkv.view(b, n, 3, heads, dh)[:, :, 2].permute(0, 2, 1, 3)
            if need:
                o, lse, planes = ops.attention(q, k, v, scale, return_planes=True)
                ctx.ops, ctx.scale, ctx.planes, ctx.meta = ops, scale, planes, (b, n, heads, dh)
                ctx.qn_dtypes = [t.dtype for t in qn]
                ctx.save_for_backward(o, lse, cs, qkv, res[1], *(tabs or ()))
                return o
            return ops.attention(q, k, v, scale)
        if cs is not None:
            ops.rope_apply_(qkv[..., 0:2 * heads * dh].unflatten(-1, (2 * heads, dh)), cs)     # q and k heads in one launch
        q5 = qkv.view(b, n, 3, heads, dh)
        q, k, v = (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        if ctx.needs_input_grad[0]:
            o, lse, planes = ops.attention(q, k, v, scale, return_planes=True)
            ctx.ops, ctx.scale, ctx.planes, ctx.meta = ops, scale, planes, (b, n, heads, dh)
            ctx.save_for_backward(o, lse, cs)
            return o
        return ops.attention(q, k, v, scale)

    @staticmethod
    def backward(ctx, g):
        o, lse, cs = ctx.saved_tensors[:3]
        b, n, heads, dh = ctx.meta
        buf = torch.empty(3, b, heads, n, dh, dtype=o.dtype, device=o.device)
        ctx.ops.attention_bwd(ctx.planes, o, g.contiguous(), lse, ctx.scale, heads, n, out=(buf[0], buf[1], buf[2]))
        dqkv = torch.empty(b, n, 3, heads, dh, dtype=o.dtype, device=o.device)
        dqkv.copy_(buf.permute(1, 3, 0, 2, 4))
        dqkv = dqkv.view(b, n, 3 * heads * dh)
        if ctx.norm is not None:
            qkv, stat = ctx.saved_tensors[3:5]
            grads = ctx.ops.qk_norm_bwd_(dqkv, qkv, stat, 2 * heads, heads, ctx.norm[0], ctx.saved_tensors[5:] or None, cs)
            return (dqkv, None, None, None, None, None) + _qn_grads(grads, ctx.qn_dtypes)
        if cs is not None:
            ctx.ops.rope_apply_(dqkv[..., 0:2 * heads * dh].unflatten(-1, (2 * heads, dh)), cs, transpose=True)
        return dqkv, None, None, None, None, None


class _CrossAttnFn(torch.autograd.Function):
    """The training path of the cross-attention core as one autograd node: q (B, N, H*dh) and the fused key / value projection
    kv (B, M, 2*Hkv*dh) in, merged heads out; the backward assembles dkv with one strided copy (see _SelfAttnFn).
    With qk_norm (norm, qn as in _SelfAttnFn) q and the k half of kv are normalised into buffers of their own; the raw projections stay."""

    @staticmethod
    def forward(ctx, q2, kv, heads, kv_heads, dh, scale, norm=None, *qn):
        ops = _ops()
        b, n, _ = q2.shape
        m = kv.shape[1]
        need = any(ctx.needs_input_grad)
        ctx.norm = norm
        saved = ()
        kvc = kv.contiguous()
        kv5 = kvc.view(b, m, 2, kv_heads, dh)
        v = kv5[:, :, 1].permute(0, 2, 1, 3)
        if norm is not None:
            mode, tabs = norm
            q2c = q2.contiguous()
            qn_ = torch.empty_like(q2c)
            kn_ = torch.empty(b, m, kv_heads * dh, dtype=kv.dtype, device=kv.device)
            rq = ops.qk_norm(q2c, heads, heads, mode, tabs, None, out=qn_, save_stats=need)
            rk = ops.qk_norm(kvc, kv_heads, 0, mode, tabs, None, out=kn_, save_stats=need)
            q = qn_.view(b, n, heads, dh).permute(0, 2, 1, 3)
            k = kn_.view(b, m, kv_heads, dh).permute(0, 2, 1, 3)
            if need:
                saved = (q2c, kvc, rq[1], rk[1]) + tuple(tabs or ())
            ctx.qn_dtypes = [t.dtype for t in qn]
        else:
            q = q2.view(b, n, heads, dh).permute(0, 2, 1, 3)
            k = kv5[:, :, 0].permute(0, 2, 1, 3)
        if need:
            o, lse, planes = ops.attention(q, k, v, scale, return_planes=True)
            ctx.ops, ctx.scale, ctx.planes, ctx.meta = ops, scale, planes, (b, n, m, heads, kv_heads, dh)
            ctx.save_for_backward(o, lse, *saved)
            return o
        return ops.attention(q, k, v, scale)

    @staticmethod
    def backward(ctx, g):
        o, lse = ctx.saved_tensors[:2]
        b, n, m, heads, kv_heads, dh = ctx.meta
        buf = torch.empty(2, b, kv_heads, m, dh, dtype=o.dtype, device=o.device)
        dq = torch.empty(b, heads, n, dh, dtype=o.dtype, device=o.device)
        ctx.ops.attention_bwd(ctx.planes, o, g.contiguous(), lse, ctx.scale, kv_heads, m, out=(dq, buf[0], buf[1]))
        dq2 = torch.empty(b, n, heads, dh, dtype=o.dtype, device=o.device)
        dq2.copy_(dq.permute(0, 2, 1, 3))
        dkv = torch.empty(b, m, 2, kv_heads, dh, dtype=o.dtype, device=o.device)
        dkv.copy_(buf.permute(1, 3, 0, 2, 4))
        dq2, dkv = dq2.view(b, n, heads * dh), dkv.view(b, m, 2 * kv_heads * dh)
        if ctx.norm is not None:
            q2, kv, sq, sk = ctx.saved_tensors[2:6]
            tabs = ctx.saved_tensors[6:] or None
            gq = ctx.ops.qk_norm_bwd_(dq2, q2, sq, heads, heads, ctx.norm[0], tabs, None)
            gk = ctx.ops.qk_norm_bwd_(dkv, kv, sk, kv_heads, 0, ctx.norm[0], tabs, None)
            grads = (gq[0], gq[1], gk[2], gk[3]) if gq is not None else None
            return (dq2, dkv, None, None, None, None, None) + _qn_grads(grads, ctx.qn_dtypes)
        return dq2, dkv, None, None, None, None, None


def _qn_grads(grads, dtypes):
    """The q_norm / k_norm parameter gradients of a qk_norm_bwd_ call in the parameters' dtypes ("l2": there are no parameters)."""
    if grads is None:
        return ()
    return tuple(g.to(dt) for g, dt in zip(grads, dtypes))


class _QKNormFn(torch.autograd.Function):
    """qk_norm (+ rotary) on the first nh heads of a (B, N, C) projection as a node of its own — the unfused path (train_fused_nodes
    off), where it takes the place of _RopeQKFn.  The columns past the normalised heads (v) are copied through."""

    @staticmethod
    def forward(ctx, x, cs, nh, hq, norm, *qn):
        ops = _ops()
        mode, tabs = norm
        x = x.contiguous()
        out = torch.empty_like(x)
        if x.shape[-1] > nh * 64:
            out[..., nh * 64:] = x[..., nh * 64:]
        need = any(ctx.needs_input_grad)
        res = ops.qk_norm(x, nh, hq, mode, tabs, cs, out=out, save_stats=need)
        if need:
            ctx.save_for_backward(x, res[1], cs, *(tabs or ()))
            ctx.meta = (nh, hq, mode, ops, [t.dtype for t in qn])
        return out

    @staticmethod
    def backward(ctx, g):
        x, stat, cs = ctx.saved_tensors[:3]
        nh, hq, mode, ops, dtypes = ctx.meta
        g = g.clone(memory_format=torch.contiguous_format)
        grads = ops.qk_norm_bwd_(g, x, stat, nh, hq, mode, ctx.saved_tensors[3:] or None, cs)
        if grads is not None:      # a pair no head of this call uses gets no gradient from it
            return (g, None, None, None, None) + tuple(t.to(dt) if t is not None else None for t, dt in zip(grads, dtypes))
        return (g, None, None, None, None)


class QKLayerNorm(nn.Module):
    """q_norm / k_norm of Attention(qk_norm="ln"): nn.LayerNorm(dim_heads, elementwise_affine=True, eps=1e-6) of the reference
    (transformer.py:375-376) — same parameter names (weight, bias), ones / zeros at construction, one set shared by all heads.
    It has no forward of its own: the normalisation runs inside the attention's kernels, which read fp32 tables (_as_f32)."""

    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps
        self._f32_cache = {}

    def _as_f32(self, name):
        """fp32, 16-byte aligned copy of a parameter for the kernels (LayerNorm._as_f32): the parameter itself when it already is both,
        else a converted copy cached until the parameter changes (in-place version counter / storage / epoch)."""
        t = getattr(self, name)
        if t.dtype == torch.float32 and t.data_ptr() % 16 == 0 and t.is_contiguous():
            return t.detach()
        if not _caches.trackable(t):
            return t.detach().float().clone()
        key = (t.data_ptr(), _caches.version_of(t), t.device, _caches.epoch_of(t))
        hit = self._f32_cache.get(name)
        if hit is None or hit[0] != key:
            hit = (key, t.detach().float().clone())
            self._f32_cache[name] = hit
        return hit[1]


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xin):
        xin = xin.contiguous()
        ctx.save_for_backward(xin)
        ctx.ops = _ops()
        return ctx.ops.swiglu(xin)

    @staticmethod
    def backward(ctx, g):
        (xin,) = ctx.saved_tensors
        return ctx.ops.swiglu_bwd(xin, g.contiguous())


class _GateResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gate, res):
        ops = _ops()
        x = x.contiguous()
        ctx.ops = ops
        ctx.save_for_backward(x, gate)
        return ops.gate_residual(x, gate, res.contiguous())

    @staticmethod
    def backward(ctx, g):
        x, gate = ctx.saved_tensors
        g = g.contiguous()
        dx, dgate = ctx.ops.gate_residual_bwd(g, x, gate)
        return dx, dgate.to(gate.dtype), g


class GLU(nn.Module):
    def __init__(self, dim_in, dim_out, activation=None, use_conv=False, conv_kernel_size=3):
        super().__init__()
        if use_conv:
            raise NotImplementedError("GLU(use_conv=True) is not used by the DiT and not implemented")
        self.proj = Linear(dim_in, dim_out * 2)

    def forward(self, x):
        return self.proj(x, mode="swiglu")       # x * silu(gate) in the GEMM epilogue (transformer.py:274-275)


class FeedForward(nn.Module):
    def __init__(self, dim, dim_out=None, mult=4, no_bias=False, glu=True, use_conv=False, conv_kernel_size=3,
                 zero_init_output=True):
        super().__init__()
        if not glu or use_conv:
            raise NotImplementedError("only the SwiGLU feed-forward (glu=True, use_conv=False) is implemented")
        inner_dim = int(dim * mult)
        dim_out = dim if dim_out is None else dim_out
        linear_in = GLU(dim, inner_dim)
        linear_out = Linear(inner_dim, dim_out, bias=not no_bias)
        if zero_init_output:
            nn.init.zeros_(linear_out.weight)
            if not no_bias:
                nn.init.zeros_(linear_out.bias)
        self.ff = nn.Sequential(linear_in, nn.Identity(), linear_out, nn.Identity())

    def forward(self, x, res=None, out_scale=None):
        """res: the residual stream — added in the output projection's epilogue (x = x + ff(...), transformer.py:711).
        out_scale: a LayerScale's parameter, folded into the output projection's rows and bias (Linear.forward; inference only)."""
        return self.ff[2](self.ff[0](x), res=res, out_scale=out_scale)


def _sliding_window(window):
    """None, or a sliding window as the tuple (left, right) of integers >= -1 (flash-attn's window_size; -1 = unbounded): query i sees
    key j iff (left < 0 or j >= i - left) and (right < 0 or j <= i + right).  Anything else is a ValueError."""
    if window is None:
        return None
    try:
        ok = len(window) == 2 and all(not isinstance(w, bool) and int(w) == w for w in window)
    except (TypeError, ValueError):
        ok = False
    if not ok or min(int(w) for w in window) < -1:
        raise ValueError(f"sliding_window must be a pair of integers [left, right], each >= -1 (-1 = unbounded), got {window!r}")
    return int(window[0]), int(window[1])


class Attention(nn.Module):
    def __init__(self, dim, dim_heads=64, dim_context=None, causal=False, zero_init_output=True, qk_norm="none",
                 differential=False, feat_scale=False):
        super().__init__()
        if causal or differential or feat_scale:
            raise NotImplementedError("causal / differential / feat_scale attention are not on the HIP path")
        if qk_norm not in ("l2", "ln", "dyt", "none"):
            raise ValueError(f'qk_norm must be one of ["l2", "ln", "none"], got {qk_norm}')
        if qk_norm == "dyt":
            raise NotImplementedError('qk_norm="dyt" (DynamicTanh) is not on the HIP path; "ln" and "l2" are')
        if dim_heads not in (64, 128):
            raise NotImplementedError("the HIP attention kernels serve head dim 64 (every Stable Audio DiT config; training and inference) "
                                      "and head dim 128 (inference only)")
        self.dim, self.dim_heads = dim, dim_heads
        dim_kv = dim_context if dim_context is not None else dim
        self.num_heads = dim // dim_heads
        self.kv_heads = dim_kv // dim_heads
        if dim_context is not None:
            self.to_q = Linear(dim, dim, bias=False)
            self.to_kv = Linear(dim_kv, dim_kv * 2, bias=False)
        else:
            self.to_qkv = Linear(dim, dim * 3, bias=False)
        self.to_out = Linear(dim, dim, bias=False)
        if zero_init_output:
            nn.init.zeros_(self.to_out.weight)
        self.qk_norm = qk_norm
        if qk_norm == "ln":
            self.q_norm = QKLayerNorm(dim_heads, eps=1.0e-6)
            self.k_norm = QKLayerNorm(dim_heads, eps=1.0e-6)
        self.causal = False
        self.scale = dim_heads ** -0.5

    def _norm(self):
        """(mode, fp32 tables (q gamma, q beta, k gamma, k beta) or None) for the kernels, or None without qk_norm."""
        if self.qk_norm == "none":
            return None
        if self.qk_norm == "l2":
            return ("l2", None)
        return ("ln", (self.q_norm._as_f32("weight"), self.q_norm._as_f32("bias"), self.k_norm._as_f32("weight"), self.k_norm._as_f32("bias")))

    def _norm_params(self):
        return (self.q_norm.weight, self.q_norm.bias, self.k_norm.weight, self.k_norm.bias) if self.qk_norm == "ln" else ()

    @staticmethod
    def _heads(ops, lin, x2, cs, heads, nb, ntok, sec0, nsec, tag, norm=None):
        """Input projection straight into attention operand planes (bf16, or fp8 operands when the layer is switched to fp8);
        norm (Attention._norm): q / k heads normalised in the same epilogue."""
        if norm is not None:      # (never fp8: Attention.forward refuses an fp8 input projection under qk_norm)
            return ops.gemm_heads_bf16(x2, lin.lowp_weight(), cs, heads, nb, ntok, sec0, nsec, reuse=tag, qk_norm=norm[0], norm_tables=norm[1])
        if isinstance(x2, _linear.Fp8Rows):
            qw, sw = lin.fp8_weight()
            alpha, calpha = _linear.fp8_scales(None, sw)
            return ops.gemm_heads_fp8(x2.q, qw, alpha, cs, heads, nb, ntok, sec0, nsec, reuse=tag, row_alpha=x2.scale, col_alpha=calpha)
        if lin.fp8 and lin.fp8_weight() is not None:
            qw, sw = lin.fp8_weight()
            if _linear.fp8_row_scales and x2.shape[1] % 8 == 0 and x2.stride(0) % 8 == 0 and x2.shape[1] <= 8192:
                qx, rs = ops.quant_fp8_rows(x2)
                alpha, calpha = _linear.fp8_scales(None, sw)
                return ops.gemm_heads_fp8(qx, qw, alpha, cs, heads, nb, ntok, sec0, nsec, reuse=tag, row_alpha=rs, col_alpha=calpha)
            qx, sx = ops.quant_fp8(x2)
            alpha, calpha = _linear.fp8_scales(sx, sw)
            return ops.gemm_heads_fp8(qx, qw, alpha, cs, heads, nb, ntok, sec0, nsec, reuse=tag, col_alpha=calpha)
        return ops.gemm_heads_bf16(x2, lin.lowp_weight(), cs, heads, nb, ntok, sec0, nsec, reuse=tag)

    def _forward_hd128(self, x, kv_input, rotary_pos_emb, res, norm, window=None, out_scale=None):
        """Head dim 128 (inference only; fp32 and bf16): projection through the Linear, then the standalone norm + rotary kernel
        (sat_qk_norm_fwd_hd) or the in-place rotary, then plane preparation and the forward kernel of csrc/attention.hip at D = 128
        (ops.attention), then to_out with the residual epilogue.  The projection-epilogue fusion of the head dim 64 bf16 path
        (gemm_heads_bf16) is not built at 128.
        Nothing below depends on the head dim: the fp32 no-grad self-attention under a sliding window (`window`, checked by forward)
        takes this path at head dim 64 too."""
        if torch.is_grad_enabled():
            raise NotImplementedError("head dim 128 is inference-only (there are no backward kernels at this head dim): run the model under torch.no_grad()")
        cross = hasattr(self, "to_q")
        first = self.to_q if cross else self.to_qkv
        if isinstance(x, _linear.Fp8Rows) or first.fp8 or (cross and self.to_kv.fp8):
            raise NotImplementedError("head dim 128 on an fp8 input projection is not built (keep to_qkv / to_q / to_kv in bf16)")
        ops = _ops()
        h, kv_h, dh = self.num_heads, self.kv_heads, self.dim_heads
        b, n, _ = x.shape
        if cross:
            m = kv_input.shape[1]
            q2, kv = self.to_q(x).contiguous(), self.to_kv(kv_input).contiguous()
            if norm is not None:
                mode, tabs = norm
                q2 = ops.qk_norm(q2, h, h, mode, tabs, None, head_dim=dh)
                kn = torch.empty(b, m, kv_h * dh, dtype=kv.dtype, device=kv.device)
                k2 = ops.qk_norm(kv, kv_h, 0, mode, tabs, None, out=kn, head_dim=dh)
            else:
                k2 = kv[..., :kv_h * dh]
            q = q2.view(b, n, h, dh).permute(0, 2, 1, 3)
            k = k2.unflatten(-1, (kv_h, dh)).permute(0, 2, 1, 3)
            v = kv[..., kv_h * dh:].unflatten(-1, (kv_h, dh)).permute(0, 2, 1, 3)
        else:
            cs = rotary_pos_emb[0] if rotary_pos_emb is not None else None
            qkv = self.to_qkv(x).contiguous()
            hd = h * dh
            if norm is not None:
                mode, tabs = norm
                qk = torch.empty(b, n, 2 * hd, dtype=qkv.dtype, device=qkv.device)
                ops.qk_norm(qkv, 2 * h, h, mode, tabs, cs, out=qk, head_dim=dh)
            else:
                qk = qkv[..., :2 * hd]
                if cs is not None:      # in place on the projection's own output: nothing else reads it
                    ops.rope_apply_(qk.unflatten(-1, (2 * h, dh)), cs)
            q = qk[..., :hd].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
            k = qk[..., hd:].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
            v = qkv[..., 2 * hd:].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
        return self.to_out(ops.attention(q, k, v, self.scale, window=window), res=res, out_scale=out_scale)

    def forward(self, x, context=None, rotary_pos_emb=None, causal=None, res=None, flash_attn_sliding_window=None, out_scale=None,
                **unsupported):
        """res: the residual stream, added in the output projection's epilogue (x = x + attn(...), transformer.py:703-707).
        flash_attn_sliding_window: (left, right), flash-attn's window_size (transformer.py:436) — self-attention under torch.no_grad()
        only; applied always (the reference drops it with a warning where the flash-attn package is missing, transformer.py:414-415).
        out_scale: a LayerScale's parameter, folded into to_out's rows (Linear.forward; inference only)."""
        for k, v in unsupported.items():
            if v is not None:
                raise NotImplementedError(f"Attention.forward({k}=...) is not on the HIP path")
        h, kv_h, dh = self.num_heads, self.kv_heads, self.dim_heads
        b, n, _ = x.shape
        cross = hasattr(self, "to_q")
        if cross and rotary_pos_emb is not None:
            raise NotImplementedError("rotary on a separate-projection attention is never used by the DiT")
        kv_input = context if (cross and context is not None) else x
        first = self.to_q if cross else self.to_qkv
        norm = self._norm()
        if norm is not None and (isinstance(x, _linear.Fp8Rows) or first.fp8 or (cross and self.to_kv.fp8)):
            raise NotImplementedError("qk_norm on an fp8 input projection: the fp8 heads GEMM has no norm epilogue (keep to_qkv / to_q / to_kv in bf16)")
        window = _sliding_window(flash_attn_sliding_window)
        if window is not None:
            if cross:
                raise NotImplementedError("a sliding window on cross-attention is not built (the window is self-attention only: Nq == Nk)")
            if torch.is_grad_enabled():
                raise NotImplementedError("the sliding window is inference-only (there is no windowed backward kernel; training with a "
                                          "window is not built): run the model under torch.no_grad()")
            if isinstance(x, _linear.Fp8Rows) or first.fp8:
                raise NotImplementedError("a sliding window on an fp8 input projection is not built (keep to_qkv in bf16)")
            window = _ops().attn_window(window, n, n)      # None when it hides nothing at this length: the dense paths, bit for bit
        if dh == 128:
            return self._forward_hd128(x, kv_input, rotary_pos_emb, res, norm, window, out_scale)
        if window is not None and not (_lowp(x, first.weight) and first.lowp_weight() is not None):
            return self._forward_hd128(x, kv_input, rotary_pos_emb, res, norm, window, out_scale)      # fp32: the standalone kernels, at head dim 64
        if not torch.is_grad_enabled() and _lowp(x, first.weight) and first.lowp_weight() is not None \
                and (not cross or self.to_kv.lowp_weight() is not None):
            # inference, bf16: head split, rotary and the attention kernel's operand planes come straight out of the
            # projection GEMM's epilogue (no qkv tensor, no rotary pass, no plane-preparation pass)
            ops = _ops()
            if isinstance(x, _linear.Fp8Rows):
                x2 = x
            else:
                x2 = x.reshape(b * n, -1)
                x2 = x2 if x2.dtype == torch.bfloat16 else ops.cast_bf16(x2.contiguous())
            if cross:
                m = kv_input.shape[1]
                pq = self._heads(ops, self.to_q, x2, None, h, b, n, 0, 1, "cross", norm)
                # the conditioning is the same tensor at every sampler step (dit.py caches its embedding): its K / V planes are
                # computed once per (context object, version, weight version) and kept in this layer's own buffers
                w = self.to_kv.weight
                can_cache = _caches.trackable(kv_input, w)    # an inference tensor carries no version counter: project it every call
                key = (_caches.version_of(kv_input), _caches.version_of(w), w.data_ptr(), _caches.epoch_of(w), bool(self.to_kv.fp8),
                       tuple(kv_input.shape), kv_input.dtype)
                if self.qk_norm == "ln":     # the K planes hold k_norm's output: a changed norm parameter must not keep them
                    kw, kb = self.k_norm.weight, self.k_norm.bias
                    can_cache = can_cache and _caches.trackable(kw, kb)
                    key += (_caches.version_of(kw), kw.data_ptr(), _caches.version_of(kb), kb.data_ptr(), _caches.epoch_of(kw, kb))
                hit = can_cache and getattr(self, "_kv_ctx", None) is kv_input and self._kv_key == key
                if hit:
                    pkv = self._kv_planes
                else:
                    c2 = kv_input.reshape(b * m, -1)
                    c2 = c2 if c2.dtype == torch.bfloat16 else ops.cast_bf16(c2.contiguous())
                    pkv = self._heads(ops, self.to_kv, c2, None, kv_h, b, m, 1, 2, ("crosskv", id(self)), norm)
                    if can_cache:
                        self._kv_ctx, self._kv_key, self._kv_planes = kv_input, key, pkv
                    else:
                        self.__dict__.pop("_kv_ctx", None)
                out = ops.attention_planes(pq["q"], pkv["k"], pkv["v_tr"], n, m, self.scale)
            else:
                cs = rotary_pos_emb[0] if rotary_pos_emb is not None else None
                pl = self._heads(ops, self.to_qkv, x2, cs, h, b, n, 0, 3, "self", norm)
                out = ops.attention_planes(pl["q"], pl["k"], pl["v_tr"], n, n, self.scale, window=window)
            return self.to_out(out, res=res, out_scale=out_scale)
        if _ops().train_fused_nodes and dh == 64:
            if cross:
                out = _CrossAttnFn.apply(self.to_q(x), self.to_kv(kv_input), h, kv_h, dh, self.scale, norm, *self._norm_params())
            else:
                cs = rotary_pos_emb[0] if rotary_pos_emb is not None else None
                out = _SelfAttnFn.apply(self.to_qkv(x), cs, h, dh, self.scale, norm, *self._norm_params())     # (B, N, H*dh): heads already merged
            return self.to_out(out, res=res, out_scale=out_scale)
        if cross:
            q2 = self.to_q(x)
            kv = self.to_kv(kv_input)
            if norm is not None:
                q2 = _QKNormFn.apply(q2, None, h, h, norm, *self._norm_params())
                kv = _QKNormFn.apply(kv, None, kv_h, 0, norm, *self._norm_params())
            q = q2.view(b, n, h, dh).permute(0, 2, 1, 3)
            k = kv[..., :kv_h * dh].unflatten(-1, (kv_h, dh)).permute(0, 2, 1, 3)
            v = kv[..., kv_h * dh:].unflatten(-1, (kv_h, dh)).permute(0, 2, 1, 3)
        else:
            qkv = self.to_qkv(x)
            if norm is not None:
                qkv = _QKNormFn.apply(qkv, rotary_pos_emb[0] if rotary_pos_emb is not None else None, 2 * h, h, norm, *self._norm_params())
            elif rotary_pos_emb is not None:
                cs, _ = rotary_pos_emb
                qkv = _RopeQKFn.apply(qkv, cs, h, dh)
            hd = h * dh
            q = qkv[..., 0:hd].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
            k = qkv[..., hd:2 * hd].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
            v = qkv[..., 2 * hd:].unflatten(-1, (h, dh)).permute(0, 2, 1, 3)
        out = _AttentionCoreFn.apply(q, k, v, self.scale)       # (B, N, H*dh): heads already merged
        return self.to_out(out, res=res, out_scale=out_scale)


class LayerScale(nn.Module):
    """The per-channel scale of a residual branch (transformer.py:243-248): one parameter `scale`, 1e-5 at construction.  Standalone
    forward for API parity; inside TransformerBlock the multiply never runs — the scale is folded into the branch's output projection
    (Linear.forward(out_scale=...)), inference only."""

    def __init__(self, dim, init_val=1e-5):
        super().__init__()
        self.scale = nn.Parameter(torch.full([dim], init_val))

    def forward(self, x):
        return x * self.scale


def _fp8_rows_for(attn, lin):
    """The projection a LayerNorm may hand fp8-quantised rows to (LayerNorm.forward(fp8_for=...)): none at head dim 128, whose input
    projections are plain Linears (Attention._forward_hd128 takes no Fp8Rows)."""
    return lin if attn.dim_heads == 64 else None


class TransformerBlock(nn.Module):
    def __init__(self, dim, dim_heads=64, cross_attend=False, dim_context=None, global_cond_dim=None, causal=False,
                 zero_init_branch_outputs=True, conformer=False, layer_ix=-1, remove_norms=False, add_rope=False,
                 layer_scale=False, attn_kwargs={}, ff_kwargs={}, norm_kwargs={}):
        super().__init__()
        if conformer or remove_norms or causal:
            raise NotImplementedError("conformer / remove_norms / causal are not on the HIP path")
        self.dim = dim
        self.dim_heads = min(dim_heads, dim)
        self.cross_attend = cross_attend
        self.dim_context = dim_context
        if layer_scale:      # the scales start at 1e-5: zero-initialised branches on top would be redundant (transformer.py:609-611)
            zero_init_branch_outputs = False
        self.layer_scale = bool(layer_scale)
        self.add_rope = bool(add_rope)
        self.pre_norm = LayerNorm(dim, **norm_kwargs)
        self.self_attn = Attention(dim, dim_heads=self.dim_heads, zero_init_output=zero_init_branch_outputs, **attn_kwargs)
        self.self_attn_scale = LayerScale(dim) if layer_scale else nn.Identity()
        if cross_attend:
            self.cross_attend_norm = LayerNorm(dim, **norm_kwargs)
            self.cross_attn = Attention(dim, dim_heads=self.dim_heads, dim_context=dim_context,
                                        zero_init_output=zero_init_branch_outputs, **attn_kwargs)
            self.cross_attn_scale = LayerScale(dim) if layer_scale else nn.Identity()
        self.ff_norm = LayerNorm(dim, **norm_kwargs)
        self.ff = FeedForward(dim, zero_init_output=zero_init_branch_outputs, **ff_kwargs)
        self.ff_scale = LayerScale(dim) if layer_scale else nn.Identity()
        self.layer_ix = layer_ix
        self.global_cond_dim = global_cond_dim
        if global_cond_dim is not None:
            self.to_scale_shift_gate = nn.Parameter(torch.randn(6 * dim) / dim ** 0.5)
        # a rotary table of the block's own (transformer.py:656), used when the caller hands none in (:672-673)
        self.rope = RotaryEmbedding(self.dim_heads // 2) if add_rope else None

    def _forward_layer_scale(self, x, context, global_cond, rotary_pos_emb, sw):
        """layer_scale=True, inference: x = x + scale * branch(...) (transformer.py:704-712), under adaLN x = branch * sigmoid(1 - gate) *
        scale + x (:684-686, :699-701).  The scale is folded into each branch's output projection (Linear.forward(out_scale=...)), so
        the block runs the launches of the block without it: the residual add stays in the GEMM epilogue, the gate in _GateResidualFn."""
        if torch.is_grad_enabled():
            raise NotImplementedError("TransformerBlock(layer_scale=True) is inference-only (the scale is folded into the output projections and "
                                      "has no gradient): run the model under torch.no_grad()")
        d = self.dim
        s_attn, s_ff = self.self_attn_scale.scale, self.ff_scale.scale
        if self.global_cond_dim is not None and self.global_cond_dim > 0 and global_cond is not None:
            mod = (self.to_scale_shift_gate + global_cond).to(x.dtype).contiguous()   # (B, 6D)
            scale_self, shift_self, gate_self = mod[:, 0:d], mod[:, d:2 * d], mod[:, 2 * d:3 * d]
            scale_ff, shift_ff, gate_ff = mod[:, 3 * d:4 * d], mod[:, 4 * d:5 * d], mod[:, 5 * d:6 * d]
            h = self.self_attn(self.pre_norm(x, scale_self, shift_self), rotary_pos_emb=rotary_pos_emb, flash_attn_sliding_window=sw, out_scale=s_attn)
            x = _GateResidualFn.apply(h, gate_self, x)
            if context is not None and self.cross_attend:
                x = self.cross_attn(self.cross_attend_norm(x), context=context, res=x, out_scale=self.cross_attn_scale.scale)
            h = self.ff(self.ff_norm(x, scale_ff, shift_ff), out_scale=s_ff)
            return _GateResidualFn.apply(h, gate_ff, x)
        x = self.self_attn(self.pre_norm(x), rotary_pos_emb=rotary_pos_emb, res=x, flash_attn_sliding_window=sw, out_scale=s_attn)
        if context is not None and self.cross_attend:
            x = self.cross_attn(self.cross_attend_norm(x), context=context, res=x, out_scale=self.cross_attn_scale.scale)
        return self.ff(self.ff_norm(x), res=x, out_scale=s_ff)

    def forward(self, x, context=None, global_cond=None, rotary_pos_emb=None, self_attention_flash_sliding_window=None, **unsupported):
        """self_attention_flash_sliding_window: (left, right) for self_attn alone (transformer.py:683, :704; inference only);
        cross_attention_flash_sliding_window, like every other option of the reference's block forward, raises."""
        for k, v in unsupported.items():
            if v is not None:
                raise NotImplementedError(f"TransformerBlock.forward({k}=...) is not on the HIP path")
        d = self.dim
        sw = self_attention_flash_sliding_window
        if rotary_pos_emb is None and self.add_rope:
            rotary_pos_emb = self.rope.forward_from_seq_len(x.shape[-2])
        if self.layer_scale:
            return self._forward_layer_scale(x, context, global_cond, rotary_pos_emb, sw)
        if self.global_cond_dim is not None and self.global_cond_dim > 0 and global_cond is not None:
            # adaLN: (to_scale_shift_gate + global_cond).chunk(6)   (transformer.py:677)
            # cast to the activation dtype: under bf16 autocast the fp32 parameter promotes the sum to fp32 while x is bf16
            mod = (self.to_scale_shift_gate + global_cond).to(x.dtype).contiguous()   # (B, 6D)
            scale_self, shift_self, gate_self = mod[:, 0:d], mod[:, d:2 * d], mod[:, 2 * d:3 * d]
            scale_ff, shift_ff, gate_ff = mod[:, 3 * d:4 * d], mod[:, 4 * d:5 * d], mod[:, 5 * d:6 * d]
            h = self.self_attn(self.pre_norm(x, scale_self, shift_self, fp8_for=_fp8_rows_for(self.self_attn, self.self_attn.to_qkv)), rotary_pos_emb=rotary_pos_emb,
                               flash_attn_sliding_window=sw)
            x = _GateResidualFn.apply(h, gate_self, x)                           # h*sigmoid(1-gate)+x  (:684-686)
            if context is not None and self.cross_attend:
                x = self.cross_attn(self.cross_attend_norm(x, fp8_for=_fp8_rows_for(self.cross_attn, self.cross_attn.to_q)), context=context, res=x)   # never modulated (:688-689)
            h = self.ff(self.ff_norm(x, scale_ff, shift_ff, fp8_for=self.ff.ff[0].proj))
            x = _GateResidualFn.apply(h, gate_ff, x)
        else:
            # (fp8_for: each norm's only consumer — in fp8 inference the rows leave the LayerNorm kernel quantised)
            if torch.is_grad_enabled() and x.requires_grad and _ops().train_fused_nodes and _ops().ln_residual:
                # training: each norm also hands x through, so the residual path's gradient is added inside the LayerNorm backward kernel
                h, xr = self.pre_norm.with_residual(x)
                x = self.self_attn(h, rotary_pos_emb=rotary_pos_emb, res=xr, flash_attn_sliding_window=sw)
                if context is not None and self.cross_attend:
                    h, xr = self.cross_attend_norm.with_residual(x)
                    x = self.cross_attn(h, context=context, res=xr)
                h, xr = self.ff_norm.with_residual(x)
                return self.ff(h, res=xr)
            x = self.self_attn(self.pre_norm(x, fp8_for=_fp8_rows_for(self.self_attn, self.self_attn.to_qkv)), rotary_pos_emb=rotary_pos_emb, res=x,   # residual adds live in
                               flash_attn_sliding_window=sw)
            if context is not None and self.cross_attend:                                                                 # the output projections' epilogues
                x = self.cross_attn(self.cross_attend_norm(x, fp8_for=_fp8_rows_for(self.cross_attn, self.cross_attn.to_q)), context=context, res=x)
            x = self.ff(self.ff_norm(x, fp8_for=self.ff.ff[0].proj), res=x)
        return x


class ContinuousTransformer(nn.Module):
    def __init__(self, dim, depth, *, dim_in=None, dim_out=None, dim_heads=64, cross_attend=False, cond_token_dim=None,
                 final_cross_attn_ix=-1, global_cond_dim=None, causal=False, rotary_pos_emb=True,
                 zero_init_branch_outputs=True, conformer=False, use_sinusoidal_emb=False, use_abs_pos_emb=False,
                 abs_pos_emb_max_length=10000, num_memory_tokens=0, sliding_window=None, **kwargs):
        super().__init__()
        if causal or conformer or use_sinusoidal_emb or use_abs_pos_emb or num_memory_tokens:
            raise NotImplementedError("causal / conformer / abs-pos-emb / memory tokens are not on the HIP path")
        self.dim, self.depth, self.causal = dim, depth, False
        self.layers = nn.ModuleList([])
        self.project_in = Linear(dim_in, dim, bias=False) if dim_in is not None else nn.Identity()
        self.project_out = Linear(dim, dim_out, bias=False) if dim_out is not None else nn.Identity()
        self.rotary_pos_emb = RotaryEmbedding(max(dim_heads // 2, 32)) if rotary_pos_emb else None
        self.num_memory_tokens = 0
        self.global_cond_embedder = None
        if global_cond_dim is not None:
            self.global_cond_embedder = nn.Sequential(Linear(global_cond_dim, dim), nn.SiLU(), Linear(dim, dim * 6))
        self.final_cross_attn_ix = final_cross_attn_ix
        # [left, right] for every layer's self-attention (transformer.py:777, :845): validated here, kept as given (None, or the list /
        # tuple of the config); inference only — a forward in grad mode raises in Attention.forward.  Prepended tokens are ordinary
        # sequence positions, as in the reference.
        _sliding_window(sliding_window)
        self.sliding_window = sliding_window
        self.checkpointing = False      # opt-in activation recompute per layer (see forward)
        for i in range(depth):
            should_cross_attend = cross_attend and (final_cross_attn_ix == -1 or i <= final_cross_attn_ix)
            self.layers.append(TransformerBlock(dim, dim_heads=dim_heads, cross_attend=should_cross_attend,
                                                dim_context=cond_token_dim, global_cond_dim=global_cond_dim,
                                                zero_init_branch_outputs=zero_init_branch_outputs, layer_ix=i, **kwargs))

    def forward(self, x, prepend_embeds=None, global_cond=None, return_info=False, use_checkpointing=True,
                exit_layer_ix=None, **kwargs):
        """Per-layer activation checkpointing (reference: transformer.py:28-30, :840-845, always on in training) is OPTIONAL here:
        `self.checkpointing` (default False — a depth-24 N = 6145 step keeps 36 GiB at batch 1 on a 288 GB part) AND the reference's
        `use_checkpointing` kwarg must both be true; results are identical either way (tests/test_boundary.py)."""
        model_dtype = next(self.parameters()).dtype
        x = x.to(model_dtype)
        info = {"hidden_states": []}
        x = self.project_in(x)
        if prepend_embeds is not None:
            assert prepend_embeds.shape[-1] == x.shape[-1], "prepend dimension must match sequence dimension"
            x = torch.cat((prepend_embeds, x), dim=-2)
        rotary = self.rotary_pos_emb.forward_from_seq_len(x.shape[1]) if self.rotary_pos_emb is not None else None
        if global_cond is not None and self.global_cond_embedder is not None:
            global_cond = self.global_cond_embedder(global_cond)
        x = x.contiguous()
        ckpt = self.checkpointing and use_checkpointing and torch.is_grad_enabled()
        for layer_ix, layer in enumerate(self.layers):
            if ckpt:
                x = torch.utils.checkpoint.checkpoint(layer, x, rotary_pos_emb=rotary, global_cond=global_cond, use_reentrant=False,
                                                      self_attention_flash_sliding_window=self.sliding_window, **kwargs)
            else:
                x = layer(x, rotary_pos_emb=rotary, global_cond=global_cond, self_attention_flash_sliding_window=self.sliding_window, **kwargs)
            if return_info:
                info["hidden_states"].append(x)
            if exit_layer_ix is not None and layer_ix == exit_layer_ix:
                return (x, info) if return_info else x
        x = self.project_out(x)
        return (x, info) if return_info else x
