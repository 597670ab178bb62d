"""Thin, typed wrappers over the C ABI (include/ds_kernels.h) taking torch CUDA tensors.

PyTorch is used for device memory and streams only; every FLOP on the path runs in
libds_kernels.so.  All wrappers enqueue on the *current* torch stream (so they are captured by
torch.cuda.graph) and never synchronise.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import (ConvDesc, Segments, SumSegments, DS_EPI_ACCUM, DS_EPI_BIAS, DS_EPI_BNSUMS, DS_EPI_MASK, DS_EPI_RELU,  # noqa: F401
                   DS_EPI_STATS, DS_EPI_BN_RELU,
                   DS_DTYPE_BF16, DS_DTYPE_F32, DS_FP8_E4M3, DS_FP8_E5M2, DS_CONV_FWD, DS_CONV_DGRAD, DS_ARITH_F32, DS_ARITH_BF16,
                   DS_ARITH_FP8, DS_ARITH_F32X3, DS_FAM_IGEMM, DS_FAM_WINO2, DS_FAM_WINO4, DS_FAM_STEM, DS_FAM_BF16D, DS_FAM_FP8D,
                   DS_FAM_F32X3, DS_FAM_WINO4H, DS_FAM_STEM_POOL, DS_FAM_STEM_DGRAD, DS_PLAN_STEM_POOL, DS_PLAN_NO_SPLITK, DS_PLAN_NO_WINO4H, DS_PLAN_NO_WINO, DS_PLAN_NO_WINO4, DS_PLAN_NO_STEM_DIRECT, DS_PLAN_NO_BF16_DIRECT, DS_PLAN_ACT16,
                   DS_PLAN_PACKED_RGB, DS_PLAN_FP8_EVERYWHERE, DS_PLAN_FP8_WIDE_RULE)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream.  The raw-stream query is ~10x cheaper than building a
    torch.cuda.Stream object, which matters at ~900 launches per step."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """Device pointer of a tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
    return C.c_void_p(t.data_ptr())


def same_pad(n, k, s):
    """TF SAME geometry: out = ceil(n/s), extra padding goes bottom/right."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def make_segments(entries):
    """entries: list of (c_begin, c_end, address, ld[, dtype[, amax address]]) -> Segments struct (dtype: DS_DTYPE_F32
    default, or DS_DTYPE_BF16 for an activation destination kept in 16-bit storage; ld in elements; amax: device word
    that collects max(y) of the segment for an fp8 consumer)."""
    sg = Segments()
    sg.nseg = len(entries)
    for i, e in enumerate(entries):
        c0, c1, ptr, ld = e[:4]
        sg.c_begin[i], sg.c_end[i], sg.ld[i] = c0, c1, ld
        sg.ptr[i] = ptr
        sg.dtype[i] = e[4] if len(e) > 4 else DS_DTYPE_F32
        sg.amax[i] = e[5] if len(e) > 5 else None
    return sg


def act_dtype(t):
    """DS_DTYPE_* of an activation tensor (fp32, or bf16 under 16-bit activation storage)."""
    return DS_DTYPE_BF16 if t.dtype == torch.bfloat16 else DS_DTYPE_F32


class ConvPlan:
    """A ds_conv_desc plus its launch-derived constants, built once per layer."""

    def __init__(self, N, H, W, Cin, ldx, KH, KW, stride, Cout, ldz, w_tap_stride, w_n_stride, w_k_stride,
                 flip=0, fold_cin=0, flags=0, ldmask=0, pad_t=None, pad_l=None, OH=None, OW=None,
                 splits=1, z_split_stride=0, dtype=DS_DTYPE_F32):
        d = ConvDesc()
        d.dtype = dtype
        d.N, d.H, d.W, d.Cin, d.ldx = N, H, W, Cin, ldx
        d.KH, d.KW, d.stride = KH, KW, stride
        if OH is None:
            OH, pt = same_pad(H, KH, stride)
            OW, pl = same_pad(W, KW if not fold_cin else (Cin // fold_cin), stride)
            pad_t = pt if pad_t is None else pad_t
            pad_l = pl if pad_l is None else pad_l
        d.pad_t, d.pad_l, d.OH, d.OW = pad_t, pad_l, OH, OW
        d.Cout, d.ldz = Cout, ldz
        d.w_tap_stride, d.w_n_stride, d.w_k_stride = w_tap_stride, w_n_stride, w_k_stride
        d.flip, d.fold_cin, d.flags, d.ldmask = flip, fold_cin, flags, ldmask
        d.splits, d.z_split_stride = splits, z_split_stride
        self.d = d
        self.M = N * OH * OW
        self.partials = _lib.load().ds_conv_igemm_partials(C.byref(d)) if flags & (DS_EPI_STATS | DS_EPI_BNSUMS) else 0
        d.partials = self.partials      # a launch that would write another count fails instead of corrupting the stats
        # algorithmic FLOPs of one launch (2*M*N*K over the real, unpadded reduction; the folded
        # stem carries a zero 4th input channel that is not counted)
        k_alg = KH * KW * Cin if not fold_cin else KH * (Cin // fold_cin) * 3
        self.alg_flops = 2.0 * self.M * Cout * k_alg

    def enable_bnsums(self, ldy):
        """Conv2DBackpropInput whose result feeds a BatchNorm + ReLU backward: emit that layer's column sums from the
        epilogue (DS_EPI_BNSUMS; y of pixel stride `ldy` goes in as `mask`, the partials come out of `stats`).
        Returns the partial count, or 0 when the launch for this shape cannot carry the flag."""
        if not _lib.load().ds_conv_igemm_bnsums_supported(C.byref(self.d)):
            return 0
        self.d.partials = 0
        self.d.flags |= DS_EPI_BNSUMS
        self.d.ldmask = ldy
        self.partials = _lib.load().ds_conv_igemm_partials(C.byref(self.d))
        self.d.partials = self.partials
        return self.partials

    def run(self, x, w, z, bias=None, mask=None, stats=None, pivot=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        _lib.check(_lib.load().ds_conv_igemm(C.byref(self.d), x, w, z, bias, mask, stats, pivot, _stream()),
                   "ds_conv_igemm")
        if t is not None:
            t.end(self)


class ConvTimer:
    """HIP-event timing of every ds_conv_igemm launch on the stream it is launched on (bench.py)."""

    def __init__(self):
        self.records = []      # (start_event, end_event, alg_flops)
        self._start = None

    def begin(self):
        self._start = torch.cuda.Event(enable_timing=True)
        self._start.record(torch.cuda.current_stream())

    def end(self, plan):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        # (launches that also carry a max pool -- the stem with MaxPool_2a inside, the Branch_3 convs with the pooling loader --
        # are marked: their time is conv + pool, their FLOPs the conv's)
        d = getattr(plan, "d", None)
        pooled = getattr(plan, "family", None) == DS_FAM_STEM_POOL or bool(getattr(d, "pool_argmax", None))
        self.records.append((self._start, e, plan.alg_flops, pooled))

    def summary(self, pooled=None):
        """(launches, total_ms, total_flops) -- call after a device synchronise.  pooled: None = every launch, True / False =
        only the launches with / without a max pool inside."""
        recs = [r for r in self.records if pooled is None or r[3] == pooled]
        ms = sum(s.elapsed_time(e) for (s, e, _, _) in recs)
        return len(recs), ms, sum(f for (_, _, f, _) in recs)


CONV_TIMER = None      # set to a ConvTimer to time the dominant kernel


def head_gemm_plan(M, K, N, lda, ldc, w_ld, transposed_w=False, flags=0, ldmask=0, *, device):
    """gemm_plan for the batch x features GEMMs of the heads (Logits, W_fc, W_softmax and their dgrads): with M <= 512 rows
    and K >= 256 a SplitGemm (split-K + fixed-order combine with the epilogue), else the plain plan.  DS_SPLIT_GEMM=0: always
    the plain plan (A/B aid).  `device`: the engine's device (the slabs live beside its tensors, not on the current device)."""
    if M <= 512 and K >= 256 and _lib.tuning_env("DS_SPLIT_GEMM", "1") != "0":
        return SplitGemm(M, K, N, lda, ldc, w_ld, transposed_w, flags, ldmask, 8 if K >= 512 else 4, device)
    return gemm_plan(M, K, N, lda, ldc, w_ld, transposed_w=transposed_w, flags=flags, ldmask=ldmask)


def gemm_plan(M, K, N, lda, ldc, w_ld, transposed_w=False, flags=0, ldmask=0, splits=1, z_split_stride=0,
              dtype=DS_DTYPE_F32):
    """C[M,N] = A[M,K] * W (row-major W[K,N] with row stride w_ld), or * W^T when transposed_w
    (then W is [N,K] row-major): both are read in place.  splits>1: split-K, slab s of partial
    sums at C + s*z_split_stride (the consumer adds the slabs)."""
    if transposed_w:
        return ConvPlan(M, 1, 1, K, lda, 1, 1, 1, N, ldc, 0, w_ld, 1, flags=flags, ldmask=ldmask,
                        pad_t=0, pad_l=0, OH=1, OW=1, splits=splits, z_split_stride=z_split_stride, dtype=dtype)
    return ConvPlan(M, 1, 1, K, lda, 1, 1, 1, N, ldc, 0, 1, w_ld, flags=flags, ldmask=ldmask,
                    pad_t=0, pad_l=0, OH=1, OW=1, splits=splits, z_split_stride=z_split_stride, dtype=dtype)


class SplitGemm:
    """A batch x features GEMM (M <= 512 rows: one or two row tiles) as split-K ds_conv_igemm + ds_slab_epilogue: the
    single launch walks K serially in a handful of workgroups; `splits` slabs of partial sums and a fixed-order combine
    with the epilogue (bias / accumulate / mask / relu) take a third of the time.  Same call as ConvPlan.run."""

    def __init__(self, M, K, N, lda, ldc, w_ld, transposed_w, flags, ldmask, splits, device):
        self.M, self.N, self.ldc, self.flags, self.ldmask, self.splits = M, N, ldc, flags, ldmask, splits
        self.slabs = torch.empty(splits, M, N, device=device)
        self.plan = gemm_plan(M, K, N, lda, N, w_ld, transposed_w=transposed_w, splits=splits, z_split_stride=M * N)
        self.d, self.alg_flops, self.partials = self.plan.d, self.plan.alg_flops, 0

    def run(self, x, w, z, bias=None, mask=None, stats=None, pivot=None):
        if stats is not None or pivot is not None:
            raise ValueError("SplitGemm has no BatchNorm-statistics epilogue (the heads' GEMMs are not followed by BatchNorm)")
        t = CONV_TIMER
        if t is not None:
            t.begin()
        lib = _lib.load()
        _lib.check(lib.ds_conv_igemm(C.byref(self.plan.d), x, w, _p(self.slabs), None, None, None, None, _stream()),
                   "ds_conv_igemm")
        _lib.check(lib.ds_slab_epilogue(_p(self.slabs), self.splits, self.M * self.N, self.N, self.M, self.N, z, self.ldc,
                                        bias, mask, self.ldmask, self.flags, _stream()), "ds_slab_epilogue")
        if t is not None:
            t.end(self)


def slab_combine(gemm, out, ldo, flags=0, bias=None, mask=None, ldmask=0, pre=None, out2=None, ldo2=0, n_split=0):
    """ds_slab_combine of a SplitGemm's slabs into `out` (addresses; ds_slab_epilogue's arguments).  pre: a second SplitGemm
    whose combined slabs are the DS_EPI_ACCUM operand; out2 / ldo2 / n_split: columns [n_split, N) go to a second tensor."""
    c = _lib.SlabCombine()
    c.slabs, c.splits, c.slab_stride, c.lds = gemm.slabs.data_ptr(), gemm.splits, gemm.M * gemm.N, gemm.N
    if pre is not None:
        assert (pre.M, pre.N) == (gemm.M, gemm.N)
        c.pre_slabs, c.pre_splits, c.pre_slab_stride, c.pre_lds = pre.slabs.data_ptr(), pre.splits, pre.M * pre.N, pre.N
    c.M, c.N, c.flags = gemm.M, gemm.N, flags
    c.out, c.ldo, c.out2, c.ldo2, c.n_split = out, ldo, out2, ldo2, n_split
    c.bias, c.mask, c.ldmask = bias, mask, ldmask
    return c


def _addr(p):
    return p.value if isinstance(p, C.c_void_p) else p


class GemmGroup:
    """SplitGemms that do not depend on each other (at most four) as ONE ds_gemm_group launch into their own slabs and ONE
    ds_slab_epilogue_group launch of `combines` (slab_combine): the bits of the SplitGemm.run calls they replace, two launches
    on the chain instead of two per GEMM."""

    def __init__(self, gemms, combines):
        n = len(gemms)
        self.gemms, self.n = gemms, n
        self._descs = (_lib._CD * n)(*[C.pointer(g.plan.d) for g in gemms])
        self._z = (C.c_void_p * n)(*[g.slabs.data_ptr() for g in gemms])
        self._combines = (_lib.SlabCombine * len(combines))(*combines)
        self.alg_flops = sum(g.alg_flops for g in gemms)

    def run(self, xs, ws):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        lib = _lib.load()
        n = self.n
        if n == 1:      # (one problem: its own launch)
            _lib.check(lib.ds_conv_igemm(C.byref(self.gemms[0].plan.d), xs[0], ws[0], _p(self.gemms[0].slabs), None, None, None,
                                         None, _stream()), "ds_conv_igemm")
        else:
            x = (C.c_void_p * n)(*[_addr(p) for p in xs])
            w = (C.c_void_p * n)(*[_addr(p) for p in ws])
            _lib.check(lib.ds_gemm_group(self._descs, x, w, self._z, n, _stream()), "ds_gemm_group")
        _lib.check(lib.ds_slab_epilogue_group(self._combines, len(self._combines), _stream()), "ds_slab_epilogue_group")
        if t is not None:
            t.end(self)


def ce_desc(label_smoothing=0.0, class_weights=None):
    """ds_ce_desc: label_smoothing and the per-class weights (a float32 device tensor of C entries, or None).  The caller
    keeps the tensor alive for as long as the descriptor is used."""
    d = _lib.CeDesc()
    d.label_smoothing = float(label_smoothing)
    d.class_weights = None if class_weights is None else _p(class_weights).value
    return d


def split_gemm_ce(gemm, x, w, logits, bias, labels, loss, dlogits, ce=None):
    """SplitGemm.run of the W_softmax GEMM with DS_EPI_BIAS and softmax_ce(logits, labels, .., 1.0, None, loss, dlogits) behind
    it, the combine and the cross entropy as ONE single-workgroup launch (ds_slab_epilogue_ce): the same bits.  ce: a ce_desc --
    softmax_ce_opts behind the combine instead (ds_slab_epilogue_ce_opts)."""
    t = CONV_TIMER
    if t is not None:
        t.begin()
    lib = _lib.load()
    _lib.check(lib.ds_conv_igemm(C.byref(gemm.plan.d), x, w, _p(gemm.slabs), None, None, None, None, _stream()), "ds_conv_igemm")
    if t is not None:
        t.end(gemm)
    if ce is not None:
        _lib.check(lib.ds_slab_epilogue_ce_opts(C.byref(ce), _p(gemm.slabs), gemm.splits, gemm.M * gemm.N, gemm.N, gemm.M, gemm.N,
                                                _p(logits), bias, _p(labels), 1.0, None, _p(loss), _p(dlogits), _stream()),
                   "ds_slab_epilogue_ce_opts")
        return
    _lib.check(lib.ds_slab_epilogue_ce(_p(gemm.slabs), gemm.splits, gemm.M * gemm.N, gemm.N, gemm.M, gemm.N, _p(logits), bias,
                                       _p(labels), 1.0, None, _p(loss), _p(dlogits), _stream()), "ds_slab_epilogue_ce")


class WinoPlan:
    """3x3 stride-1 SAME conv through ds_conv_wino (fused Winograd F(2x2,3x3)) or, with f4, ds_conv_wino4
    (F(4x4,3x3): H, W multiples of four); `u` is the transformed filter (`u_elems` floats)."""

    def __init__(self, N, H, W, Cin, ldx, Cout, ldz, flags=0, f4=False):
        self.args = (N, H, W, Cin, ldx, Cout, ldz)
        self.flags = flags
        self.f4 = bool(f4)
        lib = _lib.load()
        self._run, self._name = (lib.ds_conv_wino4, "ds_conv_wino4") if f4 else (lib.ds_conv_wino, "ds_conv_wino")
        self._partials = lib.ds_conv_wino4_partials if f4 else lib.ds_conv_wino_partials
        self.u_elems = (36 if f4 else 16) * Cin * Cout
        self.M = N * H * W
        self.partials = self._partials(N, H, W) if flags & (DS_EPI_STATS | DS_EPI_BNSUMS) else 0
        self.alg_flops = 2.0 * self.M * Cout * 9 * Cin          # the convolution's FLOPs, not Winograd's

    def enable_bnsums(self):
        """As ConvPlan.enable_bnsums (y has the output's pixel stride)."""
        N, H, W = self.args[:3]
        self.flags = (self.flags & ~DS_EPI_STATS) | DS_EPI_BNSUMS      # (the two sum epilogues exclude each other)
        self.partials = self._partials(N, H, W)
        return self.partials

    def set_ldx(self, ldx):
        self.args = self.args[:4] + (ldx,) + self.args[5:]

    def set_ldz(self, ldz):
        self.args = self.args[:6] + (ldz,)

    def run(self, x, u, z, stats=None, pivot=None, ymask=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        N, H, W, Cin, ldx, Cout, ldz = self.args
        _lib.check(self._run(x, u, z, stats, pivot, ymask, N, H, W, Cin, ldx, Cout, ldz, self.flags, _stream()), self._name)
        if t is not None:
            t.end(self)


class LayerPlan:
    """One conv layer launch planned BY THE LIBRARY (ds_conv_plan): the engine says what the layer is -- role (forward /
    Conv2DBackpropInput), arithmetic, filter [k][k][w_cin][w_cout], map, strides of x and z, epilogue flags -- and the
    library picks the kernel family (implicit GEMM / wide 1x1, Winograd F(2x2) / F(4x4), packed-RGB stem, register-direct
    bf16 / fp8 / f32x3), sizes the BatchNorm partials and names the prepared filter form.  `d` is the live descriptor
    (ldx, ldz, flags, norm_* / mask_* may change between runs)."""

    def __init__(self, role, arith, options, N, H, W, w_cin, w_cout, k, stride, ldx, ldz, flags=0):
        self.p = _lib.LayerPlanStruct()
        _lib.check(_lib.load().ds_conv_plan(C.byref(self.p), role, arith, options, N, H, W, w_cin, w_cout, k, stride, ldx,
                                            ldz, flags), "ds_conv_plan")
        self.d = self.p.d                    # a view into self.p
        self.family = self.p.family
        self.M = N * self.d.OH * self.d.OW
        self.alg_flops = self.p.alg_flops
        self.u = None                        # the prepared filter (alloc_weights), None: the family reads HWIO in place
        self.wscale = None
        self.io = _lib.ConvIO()
        self.ws_bytes = int(self.p.ws_bytes)     # > 0: run() needs a scratch tensor of that size (set_workspace): split-K Winograd
        self.splitk = int(self.p.splitk)
        self._ws = None
        self._run = _lib.load().ds_conv_run
        self._ref = C.byref(self.p)
        self._io_ref = C.byref(self.io)

    @property
    def partials(self):
        return self.p.partials

    @property
    def x16_ok(self):
        return bool(self.p.x16_ok)

    def alloc_weights(self, device):
        if self.p.w_bytes:
            self.u = torch.empty(self.p.w_bytes, dtype=torch.uint8, device=device)
        if self.p.wscale_floats:
            self.wscale = torch.zeros(self.p.wscale_floats, device=device)
            self.io.wscale = self.wscale.data_ptr()

    def set_workspace(self, t):
        """Scratch for plans with ws_bytes > 0 (private to the stream the plan runs on; at least ws_bytes long)."""
        assert t.numel() * t.element_size() >= self.ws_bytes
        self._ws = t
        self.io.ws, self.io.ws_bytes = t.data_ptr(), t.numel() * t.element_size()

    def prepare(self, w_hwio):
        """Filter -> the form the chosen family reads (no-op for the families that read HWIO in place)."""
        if self.u is not None:
            _lib.check(_lib.load().ds_conv_prepare_weights(self._ref, w_hwio, _p(self.u), _p(self.wscale), _stream()),
                       "ds_conv_prepare_weights")

    def enable_bnsums(self, ldy):
        """Conv2DBackpropInput whose result feeds a BatchNorm + ReLU backward: that layer's column sums from the epilogue
        (y with pixel stride ldy goes in as `mask`).  Returns the partial count, 0 when the chosen kernel cannot."""
        return int(_lib.load().ds_conv_plan_enable_bnsums(self._ref, ldy))

    def norm_supported(self):
        return bool(_lib.load().ds_conv_plan_norm_supported(self._ref))

    def enable_pool3(self, argmax):
        """Forward 1x1 conv behind a 3x3 / 1 SAME max pool (an Inception block's Branch_3): the pool is formed ON LOAD
        (ds_conv_desc.pool_argmax) -- `argmax` [N*H*W, Cin] uint8 receives the winners ds_maxpool_fwd would record and x is
        the pool's INPUT.  Returns False when the chosen kernel cannot (the caller keeps the separate pool pass)."""
        if not _lib.load().ds_conv_plan_enable_pool3(self._ref, _p(argmax)):
            return False
        self.pool_argmax = argmax            # (kept alive: the descriptor holds its address)
        return True

    def copy(self):
        """A second plan for the same launch that SHARES this plan's prepared filter and workspace: its descriptor (ldx, ldz,
        flags, on-load pointers) can be changed without touching this one."""
        q = object.__new__(LayerPlan)
        q.p = _lib.LayerPlanStruct()
        C.memmove(C.byref(q.p), self._ref, C.sizeof(q.p))
        q._ref = C.byref(q.p)
        q.d, q.family, q.M, q.alg_flops = q.p.d, q.p.family, self.M, self.alg_flops
        q.u, q.wscale, q._ws = self.u, self.wscale, self._ws
        q.io = _lib.ConvIO()
        q.io.ws, q.io.ws_bytes = self.io.ws, self.io.ws_bytes
        q.ws_bytes, q.splitk = self.ws_bytes, self.splitk
        q._run, q._io_ref = self._run, C.byref(q.io)
        q.pool_argmax = getattr(self, "pool_argmax", None)
        return q

    def bn_relu_variant(self, ldz=None):
        """copy() with the inference epilogue DS_EPI_BN_RELU (run_bn_relu: relu(acc * scale + shift) stored with pixel stride
        `ldz`, nothing else written), or None where the chosen family does not carry it for that stride.  The kernel family
        and tile are this plan's, so the accumulators are bit-identical."""
        q = self.copy()
        q.p.d.flags, q.p.d.partials, q.p.partials = 0, 0, 0
        if ldz is not None:
            q.p.d.ldz = ldz          # (the library decides on the stride the launch will use)
        if not _lib.load().ds_conv_plan_enable_bn_relu(q._ref):
            return None
        return q

    def run_bn_relu(self, x, w_hwio, y, scale, shift):
        """A bn_relu_variant() plan: y (pixel stride d.ldz) = relu(conv * scale + shift); scale / shift device addresses."""
        t = CONV_TIMER
        if t is not None:
            t.begin()
        self.io.scale, self.io.shift = scale, shift
        _lib.check(self._run(self._ref, x, w_hwio if self.u is None else self.u.data_ptr(), y, self._io_ref, _stream()),
                   "ds_conv_run")
        if t is not None:
            t.end(self)

    def enable_bn_backward_on_load(self, mean, rstd, shift, coef, parts):
        """Conv2DBackpropInput of a 1x1 conv + BatchNorm + ReLU layer straight from z and the activation gradient: the
        layer's ds_bn_bwd_apply pass is formed on load (ds_conv_desc.bnb).  parts: [(c0, c1, address, ld)] of dy.
        Returns False when the chosen kernel cannot (the caller keeps the separate pass)."""
        if not _lib.load().ds_conv_plan_bnb_supported(self._ref) or len(parts) > 3:
            return False
        if any(c0 % 16 for (c0, _, _, _) in parts):
            return False
        b = _lib.BnBwdOnLoad()
        b.mean, b.rstd, b.shift, b.coef = mean.data_ptr(), rstd.data_ptr(), shift.data_ptr(), coef.data_ptr()
        b.nseg = len(parts)
        for i, (c0, c1, ptr, ld) in enumerate(parts):
            assert c0 == (parts[i - 1][1] if i else 0)
            b.c_end[i], b.ld[i], b.dy[i] = c1, ld, ptr
        self.bnb = b                         # (kept alive: the descriptor holds its address)
        self.d.bnb = C.addressof(b)
        return True

    def run(self, x, w_hwio, z, stats=None, pivot=None, mask=None, bias=None, x_amax=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        io = self.io
        io.stats, io.pivot, io.mask, io.bias, io.x_amax = stats, pivot, mask, bias, x_amax
        _lib.check(self._run(self._ref, x, w_hwio if self.u is None else self.u.data_ptr(), z, self._io_ref, _stream()),
                   "ds_conv_run")
        if t is not None:
            t.end(self)


def conv_norm_supported(plan):
    """Would ds_conv_igemm apply ds_conv_desc.norm_rstd / norm_shift (BatchNorm + ReLU on load) for this plan?"""
    return bool(_lib.load().ds_conv_igemm_norm_supported(C.byref(plan.d)))


def wino4_supported(H, W, Cin, Cout):
    return bool(_lib.load().ds_conv_wino4_supported(H, W, Cin, Cout))


def wino4_prefer(N, H, W, Cin, Cout):
    """The library's launch-time model: is ds_conv_wino4 expected to beat ds_conv_wino on this shape?"""
    return bool(_lib.load().ds_conv_wino4_prefer(N, H, W, Cin, Cout))


def wino_transform_weights(w_ptr, u, Cin, Cout, dgrad, f4=False):
    lib = _lib.load()
    if f4:
        _lib.check(lib.ds_wino4_transform_weights(w_ptr, _p(u), Cin, Cout, int(dgrad), _stream()), "ds_wino4_transform_weights")
    else:
        _lib.check(lib.ds_wino_transform_weights(w_ptr, _p(u), Cin, Cout, int(dgrad), _stream()), "ds_wino_transform_weights")


class StemPlan:
    """Conv2d_1a_7x7 through ds_conv_stem: packed RGB input [N, H, W, 3], HWIO weights with `cin_store` input rows."""

    def __init__(self, N, H, W, cin_store, Cout, ldz, bf16=False):
        self.args = (N, H, W, cin_store, Cout, ldz)
        self.bf16 = bf16               # ds_conv_stem_bf16: operands rounded to bf16, bf16 MFMA (the 16-bit configurations)
        self.flags = DS_EPI_STATS      # kept for the common plan interface: statistics are on iff `stats` is passed
        OH, OW = (H + 1) // 2, (W + 1) // 2
        self.M = N * OH * OW
        self.partials = (_lib.load().ds_conv_stem_bf16_partials if bf16 else _lib.load().ds_conv_stem_partials)(N, OH, OW)
        self.alg_flops = 2.0 * self.M * Cout * 147

    def run(self, x, w, z, stats=None, pivot=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        N, H, W, cs, Cout, ldz = self.args
        f = _lib.load().ds_conv_stem_bf16 if self.bf16 else _lib.load().ds_conv_stem
        _lib.check(f(x, w, z, stats, pivot, N, H, W, cs, Cout, ldz, _stream()), "ds_conv_stem")
        if t is not None:
            t.end(self)


class Bf16Plan:
    """1x1 / 3x3 conv (or its dgrad) through ds_conv_bf16: register-direct bf16 MFMA, weights pre-converted by
    `weights_to_bf16` into the kernel's K-loop order.  Geometry arguments as ConvPlan's."""

    def __init__(self, N, H, W, Cin, ldx, k, stride, Cout, ldz, flags=0, pad_t=None, pad_l=None, OH=None, OW=None):
        d = ConvDesc()
        d.dtype = DS_DTYPE_BF16
        d.N, d.H, d.W, d.Cin, d.ldx = N, H, W, Cin, ldx
        d.KH, d.KW, d.stride = k, k, stride
        if OH is None:
            OH, pt = same_pad(H, k, stride)
            OW, pl = same_pad(W, k, stride)
            pad_t = pt if pad_t is None else pad_t
            pad_l = pl if pad_l is None else pad_l
        d.pad_t, d.pad_l, d.OH, d.OW = pad_t, pad_l, OH, OW
        d.Cout, d.ldz, d.flags, d.splits = Cout, ldz, flags, 1
        self.d = d
        lib = _lib.load()
        if not lib.ds_conv_bf16_supported(C.byref(d)):
            raise ValueError("ds_conv_bf16 does not take this geometry")
        self.M = N * OH * OW
        self.partials = lib.ds_conv_bf16_partials(C.byref(d)) if flags & DS_EPI_STATS else 0
        self.alg_flops = 2.0 * self.M * Cout * k * k * Cin

    def set_ldx(self, ldx):
        self.d.ldx = ldx

    @property
    def flags(self):
        return self.d.flags

    @flags.setter
    def flags(self, v):
        self.d.flags = v

    def run(self, x, wb, z, stats=None, pivot=None, mask=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        _lib.check(_lib.load().ds_conv_bf16(C.byref(self.d), x, wb, z, mask, stats, pivot, _stream()), "ds_conv_bf16")
        if t is not None:
            t.end(self)


class Fp8Plan(Bf16Plan):
    """1x1 / 3x3 conv (or its dgrad) through ds_conv_fp8: register-direct fp8 MFMA with per-tensor power-of-two scales.
    `wq`, `wscale`: the filter converted by `weights_to_fp8`; `x_amax`: device word holding max|x| (`absmax`);
    a_format: DS_FP8_E4M3 for forward activations, DS_FP8_E5M2 for gradients.  Geometry arguments as ConvPlan's."""

    def __init__(self, N, H, W, Cin, ldx, k, stride, Cout, ldz, flags=0, a_format=DS_FP8_E4M3, **kw):
        super().__init__(N, H, W, Cin, ldx, k, stride, Cout, ldz, flags=flags, **kw)
        lib = _lib.load()
        if not lib.ds_conv_fp8_supported(C.byref(self.d)):
            raise ValueError("ds_conv_fp8 does not take this geometry")
        self.a_format = a_format
        self.partials = lib.ds_conv_fp8_partials(C.byref(self.d)) if flags & DS_EPI_STATS else 0

    def run(self, x, wq, z, stats=None, pivot=None, x_amax=None, wscale=None, mask=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        _lib.check(_lib.load().ds_conv_fp8(C.byref(self.d), x, x_amax, self.a_format, wq, wscale, z, mask, stats, pivot,
                                           _stream()), "ds_conv_fp8")
        if t is not None:
            t.end(self)


AMAX_FLOATS = 512       # DS_AMAX_FLOATS: a max|.| record = 16 slots, one per 128-byte line; its value = max of the slots
WSCALE_FLOATS = 4 + AMAX_FLOATS


def amax_value(record):
    """Host value of a max|.| record (tests)."""
    return float(record.view(-1)[:AMAX_FLOATS:32].max().item())


def absmax(x, n, out, x_dtype=DS_DTYPE_F32):
    """out (a record of AMAX_FLOATS floats) <- max |x[:n]| on the device (no host sync).  x: tensor (its dtype counts) or
    raw address + x_dtype."""
    if not isinstance(x, C.c_void_p):
        x_dtype = act_dtype(x)
        x = _p(x)
    _lib.check(_lib.load().ds_absmax(x, n, x_dtype, _p(out), _stream()), "ds_absmax")


def weights_fp8_bytes(Cin, Cout, taps, dgrad):
    return int(_lib.load().ds_weights_fp8_bytes(Cin, Cout, taps, int(dgrad)))


def weights_to_fp8(w_ptr, wq, wscale, Cin, Cout, taps, dgrad):
    """HWIO fp32 filter -> ds_conv_fp8's e4m3 weight tensor `wq` + its scale record `wscale` (4 device floats)."""
    _lib.check(_lib.load().ds_weights_to_fp8(w_ptr, _p(wq), _p(wscale), Cin, Cout, taps, int(dgrad), _stream()),
               "ds_weights_to_fp8")


def weights_bf16_bytes(Cin, Cout, taps, dgrad):
    return int(_lib.load().ds_weights_bf16_bytes(Cin, Cout, taps, int(dgrad)))


def weights_to_bf16(w_ptr, wb, Cin, Cout, taps, dgrad):
    """HWIO fp32 filter -> ds_conv_bf16's weight tensor (`wb`: a uint8/bf16 device tensor of weights_bf16_bytes)."""
    _lib.check(_lib.load().ds_weights_to_bf16(w_ptr, _p(wb), Cin, Cout, taps, int(dgrad), _stream()),
               "ds_weights_to_bf16")


class F32x3Plan:
    """1x1 / 3x3 conv (or its dgrad) through ds_conv_f32x3: fp32 products on the bf16 matrix cores (every operand split into
    three bf16 pieces, six MFMAs per eight of the fp32 path; fp32-MFMA accuracy, not bit-identical).  Weights pre-split by
    `weights_to_f32x3`.  Geometry arguments as Bf16Plan's; x is fp32; d.norm_rstd / norm_shift as for ConvPlan (1x1)."""
    f4 = False

    def __init__(self, N, H, W, Cin, ldx, k, stride, Cout, ldz, flags=0, pad_t=None, pad_l=None, OH=None, OW=None):
        d = ConvDesc()
        d.dtype = DS_DTYPE_F32
        d.N, d.H, d.W, d.Cin, d.ldx = N, H, W, Cin, ldx
        d.KH, d.KW, d.stride = k, k, stride
        if OH is None:
            OH, pt = same_pad(H, k, stride)
            OW, pl = same_pad(W, k, stride)
            pad_t = pt if pad_t is None else pad_t
            pad_l = pl if pad_l is None else pad_l
        d.pad_t, d.pad_l, d.OH, d.OW = pad_t, pad_l, OH, OW
        d.Cout, d.ldz, d.flags, d.splits = Cout, ldz, flags, 1
        self.d = d
        lib = _lib.load()
        if not lib.ds_conv_f32x3_supported(C.byref(d)):
            raise ValueError("ds_conv_f32x3 does not take this geometry")
        self.M = N * OH * OW
        self.partials = lib.ds_conv_f32x3_partials(C.byref(d)) if flags & DS_EPI_STATS else 0
        self.partials_for_sums = lib.ds_conv_f32x3_partials(C.byref(d))      # what a DS_EPI_BNSUMS launch would write
        self.alg_flops = 2.0 * self.M * Cout * k * k * Cin

    def set_ldx(self, ldx):
        self.d.ldx = ldx

    def set_ldz(self, ldz):
        self.d.ldz = ldz

    @property
    def flags(self):
        return self.d.flags

    @flags.setter
    def flags(self, v):
        self.d.flags = v

    def run(self, x, wb, z, stats=None, pivot=None, mask=None):
        t = CONV_TIMER
        if t is not None:
            t.begin()
        _lib.check(_lib.load().ds_conv_f32x3(C.byref(self.d), x, wb, z, mask, stats, pivot, _stream()), "ds_conv_f32x3")
        if t is not None:
            t.end(self)


def weights_f32x3_bytes(Cin, Cout, taps, dgrad):
    return int(_lib.load().ds_weights_f32x3_bytes(Cin, Cout, taps, int(dgrad)))


def weights_to_f32x3(w_ptr, wb, Cin, Cout, taps, dgrad):
    """HWIO fp32 filter -> ds_conv_f32x3's weight tensor (three bf16 pieces per weight, K-loop order)."""
    _lib.check(_lib.load().ds_weights_to_f32x3(w_ptr, _p(wb), Cin, Cout, taps, int(dgrad), _stream()), "ds_weights_to_f32x3")


class WgradPlan:
    """dw[tap, ci, co] = sum_m x[pixel(m)+tap, ci] * dz[m, co]; geometry given by a forward ConvPlan-like desc."""

    def __init__(self, N, H, W, Cin, ldx, KH, KW, stride, Cout, lddz, pad_t=None, pad_l=None, OH=None, OW=None,
                 fold_cin=0):
        d = ConvDesc()
        d.fold_cin = fold_cin
        d.N, d.H, d.W, d.Cin, d.ldx = N, H, W, Cin, ldx
        d.KH, d.KW, d.stride = KH, KW, stride
        if OH is None:
            OH, pad_t = same_pad(H, KH, stride)
            OW, pad_l = same_pad(W, KW if not fold_cin else Cin // fold_cin, stride)
        d.pad_t, d.pad_l, d.OH, d.OW = pad_t, pad_l, OH, OW
        d.Cout, d.ldz = Cout, Cout
        self.d = d
        self.lddz = lddz
        self.ws_bytes = int(_lib.load().ds_conv_wgrad_workspace(C.byref(d)))

    def run(self, x, dz, dw, ws, ws_bytes):
        _lib.check(_lib.load().ds_conv_wgrad(C.byref(self.d), x, dz, self.lddz, dw, ws, ws_bytes, _stream()),
                   "ds_conv_wgrad")


def bn_finalize(stats, P, count, C_, beta, eps, decay, mean, rstd, shift, mm, mv, pivot=None):
    _lib.check(_lib.load().ds_bn_finalize(_p(stats), P, count, C_, _p(beta), _p(pivot), eps, decay, _p(mean),
                                          _p(rstd), _p(shift), _p(mm), _p(mv), _stream()), "ds_bn_finalize")


def bn_finalize_centered(stats, P, count, C_, beta, eps, decay, mean, rstd, shift, mm, mv, pivot, mean_c, shift_c):
    """ds_bn_finalize for a layer whose z is stored centred about the pivot: also mean - pivot and the matching shift."""
    _lib.check(_lib.load().ds_bn_finalize_centered(_p(stats), P, count, C_, _p(beta), _p(pivot), eps, decay, _p(mean), _p(rstd),
                                                   _p(shift), _p(mm), _p(mv), _p(mean_c), _p(shift_c), _stream()),
               "ds_bn_finalize_centered")


def bn_apply_relu(z, M, C_, rstd, shift, segs):
    if z.dtype == torch.bfloat16:          # z in bf16 storage (ds_conv_desc.z_dtype)
        _lib.check(_lib.load().ds_bn_apply_relu_z16(_p(z), M, C_, _p(rstd), _p(shift), C.byref(segs), _stream()),
                   "ds_bn_apply_relu_z16")
        return
    _lib.check(_lib.load().ds_bn_apply_relu(_p(z), M, C_, _p(rstd), _p(shift), C.byref(segs), _stream()),
               "ds_bn_apply_relu")


def bn_infer_prepare(beta, mm, mv, eps, C_, rstd, shift):
    _lib.check(_lib.load().ds_bn_infer_prepare(_p(beta), _p(mm), _p(mv), eps, C_, _p(rstd), _p(shift), _stream()),
               "ds_bn_infer_prepare")


class BnInferJobs:
    """ds_bn_infer_prepare_multi: (rstd, shift) of every listed BatchNorm layer from its moving statistics as ONE launch.
    jobs: (beta, moving_mean, moving_var, C, rstd, shift) tensors / int."""

    def __init__(self, jobs):
        self.n = len(jobs)
        self.arr = (_lib.BnInferJob * self.n)()
        self._keep = jobs
        for a, (beta, mm, mv, C_, rstd, shift) in zip(self.arr, jobs):
            a.beta, a.moving_mean, a.moving_var, a.C = _p(beta), _p(mm), _p(mv), C_
            a.rstd, a.shift = _p(rstd), _p(shift)

    def run(self, eps):
        _lib.check(_lib.load().ds_bn_infer_prepare_multi(C.cast(self.arr, C.c_void_p), self.n, eps, _stream()),
                   "ds_bn_infer_prepare_multi")


def bn_bwd_partials(M, C_):
    return _lib.load().ds_bn_bwd_partials(M, C_)


def bn_bwd_reduce(z, segs, M, C_, mean, rstd, shift, partials, ldz=None, z_dtype=DS_DTYPE_F32):
    """z .. partials: tensors, or raw device addresses (c_void_p) when a column sub-range of a layer is reduced
    (then z_dtype names z's storage: bf16 for a pooled activation in 16-bit storage)."""
    ptr = lambda t: t if isinstance(t, C.c_void_p) else _p(t)
    if not isinstance(z, C.c_void_p):
        z_dtype = act_dtype(z)
    _lib.check(_lib.load().ds_bn_bwd_reduce(ptr(z), C_ if ldz is None else ldz, z_dtype, C.byref(segs), M, C_, ptr(mean),
                                            ptr(rstd), ptr(shift), ptr(partials), _stream()), "ds_bn_bwd_reduce")


def bn_bwd_finalize_segs(sum_segs, M, C_, beta, dbeta, coef):
    _lib.check(_lib.load().ds_bn_bwd_finalize_segs(C.byref(sum_segs), M, C_, _p(beta), _p(dbeta), _p(coef), _stream()),
               "ds_bn_bwd_finalize_segs")


class BnFinalizeJobs:
    """ds_bn_finalize_multi: the finalizes of up to four layers as one launch.  jobs: (stats, P, count, C, beta, pivot, mean,
    rstd, shift, moving_mean, moving_var) tensors / ints; the moving statistics may be None."""

    def __init__(self, jobs):
        self.n = len(jobs)
        self.arr = (_lib.BnFinalizeJob * self.n)()
        self._keep = jobs
        for a, (stats, P, count, C_, beta, pivot, mean, rstd, shift, mm, mv) in zip(self.arr, jobs):
            a.stats, a.P, a.C, a.count = stats.data_ptr(), P, C_, count
            a.beta, a.pivot = beta.data_ptr(), (pivot.data_ptr() if pivot is not None else None)
            a.mean, a.rstd, a.shift = mean.data_ptr(), rstd.data_ptr(), shift.data_ptr()
            a.moving_mean = mm.data_ptr() if mm is not None else None
            a.moving_var = mv.data_ptr() if mv is not None else None

    def run(self, eps, decay):
        _lib.check(_lib.load().ds_bn_finalize_multi(C.cast(self.arr, C.c_void_p), self.n, eps, decay, _stream()),
                   "ds_bn_finalize_multi")


def bn_bwd_finalize_multi(sum_segs, M, C_, betas, dbetas, coef):
    """ds_bn_bwd_finalize_multi: segment i of sum_segs is a LAYER with its own beta / dbeta vector (dbetas[i] may be None)."""
    n = sum_segs.nseg
    b = (C.c_void_p * 4)(*[t.data_ptr() for t in betas[:n]])
    d = (C.c_void_p * 4)(*[(t.data_ptr() if t is not None else None) for t in dbetas[:n]])
    _lib.check(_lib.load().ds_bn_bwd_finalize_multi(C.byref(sum_segs), M, C_, C.cast(b, C.c_void_p), C.cast(d, C.c_void_p),
                                                    _p(coef), _stream()), "ds_bn_bwd_finalize_multi")


def bn_bwd_finalize(partials, P, M, C_, dbeta, coef):
    _lib.check(_lib.load().ds_bn_bwd_finalize(_p(partials), P, M, C_, _p(dbeta), _p(coef), _stream()),
               "ds_bn_bwd_finalize")


def bn_bwd_apply(z, segs, M, C_, mean, rstd, shift, coef, dz, amax=None, ldz=0):
    """dz: fp32 (over z, or any tensor with z's row stride), or a SEPARATE dense bf16 tensor [M, C] -- the form the 16-bit
    configurations' 1x1 input gradients read (ds_bn_bwd_apply_bf16)."""
    if z.dtype == torch.bfloat16:          # z in bf16 storage: dz into its own bf16 tensor
        assert dz.dtype == torch.bfloat16
        _lib.check(_lib.load().ds_bn_bwd_apply_z16(_p(z), ldz or C_, C.byref(segs), M, C_, _p(mean), _p(rstd), _p(shift),
                                                   _p(coef), _p(dz), dz.stride(0), _p(amax), _stream()), "ds_bn_bwd_apply_z16")
        return
    if dz.dtype == torch.bfloat16:
        _lib.check(_lib.load().ds_bn_bwd_apply_bf16(_p(z), ldz or C_, C.byref(segs), M, C_, _p(mean), _p(rstd), _p(shift),
                                                    _p(coef), _p(dz), dz.stride(0), _p(amax), _stream()), "ds_bn_bwd_apply_bf16")
        return
    _lib.check(_lib.load().ds_bn_bwd_apply(_p(z), ldz or C_, C.byref(segs), M, C_, _p(mean), _p(rstd), _p(shift), _p(coef),
                                           _p(dz), _p(amax), _stream()), "ds_bn_bwd_apply")


def bn_bwd_apply_cols(z, segs, M, ncols, mean, rstd, shift, coef_g, coef_gx, dz, ldz):
    """ds_bn_bwd_apply over a column range of a layer (fp32): every tensor / vector points at the range's first column, the
    two coefficient vectors come separately (their distance is the LAYER's column count, not the range's)."""
    _lib.check(_lib.load().ds_bn_bwd_apply_cols(_p(z), ldz, C.byref(segs), M, ncols, _p(mean), _p(rstd), _p(shift), _p(coef_g),
                                                _p(coef_gx), _p(dz), _stream()), "ds_bn_bwd_apply_cols")


def bn_infer_bwd_apply(z, segs, M, C_, rstd, shift, dz, ldz=0):
    """Moving-statistics BatchNorm + ReLU backward, pointwise: dz = rstd * dy * [z*rstd + shift > 0] (dz over z, or any fp32
    tensor with z's row stride).  z .. dz: tensors or raw device addresses."""
    ptr = lambda t: t if isinstance(t, C.c_void_p) else _p(t)
    _lib.check(_lib.load().ds_bn_infer_bwd_apply(ptr(z), ldz or C_, C.byref(segs), M, C_, ptr(rstd), ptr(shift), ptr(dz),
                                                 _stream()), "ds_bn_infer_bwd_apply")


def bn_infer_bwd_partials(M, C_):
    return _lib.load().ds_bn_infer_bwd_partials(M, C_)


def bn_infer_bwd_apply_sums(z, segs, M, C_, rstd, shift, dz, partials, ldz=0):
    """ds_bn_infer_bwd_apply that also emits the column sums of g = dy * [z*rstd + shift > 0] as partials [C, P],
    P = bn_infer_bwd_partials(M, C) (frozen-BatchNorm training: dbeta).  dz None: the sums only."""
    ptr = lambda t: t if isinstance(t, C.c_void_p) else _p(t)
    _lib.check(_lib.load().ds_bn_infer_bwd_apply_sums(ptr(z), ldz or C_, C.byref(segs), M, C_, ptr(rstd), ptr(shift), ptr(dz),
                                                      ptr(partials), _stream()), "ds_bn_infer_bwd_apply_sums")


class BnSumJobs:
    """ds_bn_dbeta_reduce_multi: the beta gradients of every listed layer from its partial sums as ONE launch.
    jobs: (partials address or tensor, P, C, dbeta tensor)."""

    def __init__(self, jobs):
        self.n = len(jobs)
        self.arr = (_lib.BnSumJob * self.n)()
        self._keep = jobs
        for a, (partials, P, C_, dbeta) in zip(self.arr, jobs):
            a.partials = partials if isinstance(partials, int) else partials.data_ptr()
            a.P, a.C, a.dbeta = P, C_, dbeta.data_ptr()

    def run(self):
        _lib.check(_lib.load().ds_bn_dbeta_reduce_multi(C.cast(self.arr, C.c_void_p), self.n, _stream()),
                   "ds_bn_dbeta_reduce_multi")


def maxpool_fwd(x, y, argmax, N, H, W, C_, k, stride, mode="SAME"):
    if mode == "SAME":
        OH, pt = same_pad(H, k, stride)
        OW, pl = same_pad(W, k, stride)
    else:
        OH, OW, pt, pl = (H - k) // stride + 1, (W - k) // stride + 1, 0, 0
    assert x.dtype == y.dtype
    _lib.check(_lib.load().ds_maxpool_fwd(_p(x), _p(y), _p(argmax), N, H, W, C_, k, stride, pt, pl, OH, OW,
                                          act_dtype(x), _stream()), "ds_maxpool_fwd")
    return OH, OW


def maxpool_bn_relu_fwd(z, rstd, shift, y, argmax, N, H, W, C_, k, stride, amax=None):
    """y = maxpool(relu(z*rstd + shift)) computed as relu(rstd*maxpool(z) + shift): SAME padding, 3x3 only."""
    OH, pt = same_pad(H, k, stride)
    OW, pl = same_pad(W, k, stride)
    _lib.check(_lib.load().ds_maxpool_bn_relu_fwd(_p(z), _p(rstd), _p(shift), _p(y), _p(argmax), N, H, W, C_, k, stride,
                                                  pt, pl, OH, OW, act_dtype(y), _p(amax), _stream()),
               "ds_maxpool_bn_relu_fwd")
    return OH, OW


def bn_pool_bwd_partials(N, H, W, C_):
    OH, _ = same_pad(H, 3, 2)
    OW, _ = same_pad(W, 3, 2)
    return _lib.load().ds_bn_pool_bwd_partials(N, OH, OW, C_)


def bn_pool_bwd_reduce(z, dpool, argmax, N, H, W, C_, mean, rstd, shift, partials):
    """BatchNorm(+ReLU) backward sums of a conv behind a 3x3/2 SAME max pool, from the pooled gradient."""
    OH, pt = same_pad(H, 3, 2)
    OW, pl = same_pad(W, 3, 2)
    _lib.check(_lib.load().ds_bn_pool_bwd_reduce(_p(z), _p(dpool), _p(argmax), N, H, W, C_, pt, pl, OH, OW, _p(mean),
                                                 _p(rstd), _p(shift), _p(partials), _stream()), "ds_bn_pool_bwd_reduce")


def bn_pool_bwd_apply(z, dpool, argmax, N, H, W, C_, mean, rstd, shift, coef, dz):
    OH, pt = same_pad(H, 3, 2)
    OW, pl = same_pad(W, 3, 2)
    _lib.check(_lib.load().ds_bn_pool_bwd_apply(_p(z), _p(dpool), _p(argmax), N, H, W, C_, pt, pl, OH, OW, _p(mean),
                                                _p(rstd), _p(shift), _p(coef), _p(dz), _stream()), "ds_bn_pool_bwd_apply")


def bn_pool_bwd_apply_cols(z, ldz, dz, lddz, dpool, argmax, Cp, c0, N, H, W, ncols, mean, rstd, shift, coef_g, coef_gx, k):
    """BatchNorm + ReLU backward apply of the columns [c0, c0 + ncols) of a k x k / 2 SAME max pool's input (k = 3 or 2) from the
    POOLED gradient dpool and the winners argmax [N, OH, OW, Cp]: ds_maxpool_bwd + ds_bn_bwd_apply without the full-resolution
    gradient between them, bit for bit.  z (pixel stride ldz), dz (lddz; may be z) and the per-column vectors point at the range's
    first column."""
    OH, pt = same_pad(H, k, 2)
    OW, pl = same_pad(W, k, 2)
    _lib.check(_lib.load().ds_bn_pool_bwd_apply_cols(_p(z), ldz, _p(dz), lddz, _p(dpool), _p(argmax), Cp, c0, N, H, W, pt, pl,
                                                     OH, OW, ncols, _p(mean), _p(rstd), _p(shift), _p(coef_g), _p(coef_gx), k,
                                                     _stream()), "ds_bn_pool_bwd_apply_cols")


def bn_pool_infer_bwd_apply(z, dpool, argmax, N, H, W, C_, rstd, shift, dz):
    """ds_bn_pool_bwd_apply's moving-statistics twin (conv -> BN -> ReLU -> 3x3/2 SAME pool, from the pooled gradient)."""
    OH, pt = same_pad(H, 3, 2)
    OW, pl = same_pad(W, 3, 2)
    _lib.check(_lib.load().ds_bn_pool_infer_bwd_apply(_p(z), _p(dpool), _p(argmax), N, H, W, C_, pt, pl, OH, OW, _p(rstd),
                                                      _p(shift), _p(dz), _stream()), "ds_bn_pool_infer_bwd_apply")


def bn_pool_infer_bwd_apply_sums(z, dpool, argmax, N, H, W, C_, rstd, shift, dz, partials):
    """ds_bn_pool_infer_bwd_apply that also emits the column sums of g as partials [C, P], P = bn_pool_bwd_partials(N, H, W, C)
    (frozen-BatchNorm training: dbeta).  dz None: the sums only."""
    OH, pt = same_pad(H, 3, 2)
    OW, pl = same_pad(W, 3, 2)
    _lib.check(_lib.load().ds_bn_pool_infer_bwd_apply_sums(_p(z), _p(dpool), _p(argmax), N, H, W, C_, pt, pl, OH, OW, _p(rstd),
                                                           _p(shift), _p(dz), _p(partials), _stream()),
               "ds_bn_pool_infer_bwd_apply_sums")


def maxpool_bwd(dy, argmax, dx, accumulate, N, H, W, C_, k, stride, mode="SAME"):
    if dy.dtype != torch.float32:          # (the library reads dy as floats)
        raise ValueError("maxpool_bwd: dy must be fp32, got %s" % dy.dtype)
    if mode == "SAME":
        OH, pt = same_pad(H, k, stride)
        OW, pl = same_pad(W, k, stride)
    else:
        OH, OW, pt, pl = (H - k) // stride + 1, (W - k) // stride + 1, 0, 0
    _lib.check(_lib.load().ds_maxpool_bwd(_p(dy), _p(argmax), _p(dx), int(accumulate), N, H, W, C_, k, stride, pt,
                                          pl, OH, OW, _stream()), "ds_maxpool_bwd")


def maxpool3_bwd_sums_partials(N, W, C_):
    return _lib.load().ds_maxpool3_bwd_sums_partials(N, W, C_)


def maxpool3_bwd_sums(dy, argmax, dx, accumulate, y, N, H, W, C_, partials):
    """ds_maxpool_bwd of a 3x3 / 1 SAME pool + the BatchNorm-backward sums (sum g, sum g*y over y > 0) of the activation y."""
    if dy.dtype != torch.float32:          # (the library reads dy as floats)
        raise ValueError("maxpool3_bwd_sums: dy must be fp32, got %s" % dy.dtype)
    _lib.check(_lib.load().ds_maxpool3_bwd_sums(_p(dy), _p(argmax), _p(dx), int(accumulate), _p(y), act_dtype(y), N, H, W, C_,
                                                _p(partials), _stream()), "ds_maxpool3_bwd_sums")


def avgpool_dropout_fwd(x, N, HW, C_, keep, seed, mask_in, mask_out, out, seed_dev=None):
    _lib.check(_lib.load().ds_avgpool_dropout_fwd(_p(x), N, HW, C_, keep, seed, _p(seed_dev), _p(mask_in),
                                                  _p(mask_out), _p(out), _stream()), "ds_avgpool_dropout_fwd")


def avgpool_dropout_bwd(dout, mask, N, HW, C_, keep, dx):
    _lib.check(_lib.load().ds_avgpool_dropout_bwd(_p(dout), _p(mask), N, HW, C_, keep, _p(dx), _stream()),
               "ds_avgpool_dropout_bwd")


def gather_rows(table, ids, out, B, T, D, time_major=True):
    _lib.check(_lib.load().ds_gather_rows(_p(table), _p(ids), _p(out), B, T, D, table.shape[0], int(time_major),
                                          _stream()), "ds_gather_rows")


def embedding_grad(dx, ids, dtable, B, T, D, time_major=True):
    _lib.check(_lib.load().ds_embedding_grad(_p(dx), _p(ids), _p(dtable), B, T, D, dtable.shape[0], int(time_major),
                                             _stream()), "ds_embedding_grad")


def token_dot(dx, x, seq_len, out, B, T, D):
    """out [B, T] = sum_d dx * x over time-major [T*B, D] buffers; exactly 0 at t >= seq_len[b]."""
    _lib.check(_lib.load().ds_token_dot(_p(dx), _p(x), _p(seq_len), _p(out), B, T, D, _stream()), "ds_token_dot")


def lstm_cell_fwd(gates, c_prev, h_prev, seq_len, t, B, H, forget_bias, c_out, h_out, rec_slabs=None, nslabs=0,
                  slab_stride=0):
    _lib.check(_lib.load().ds_lstm_cell_fwd(_p(gates), _p(rec_slabs), nslabs, slab_stride, _p(c_prev), _p(h_prev),
                                            _p(seq_len), t, B, H, forget_bias, _p(c_out), _p(h_out), _stream()),
               "ds_lstm_cell_fwd")


def lstm_cell_bwd(acts, c_t, c_prev, dh, dc, seq_len, t, B, H, dgates, dc_prev, dh_carry, dh_slabs=None, nslabs=0,
                  slab_stride=0):
    _lib.check(_lib.load().ds_lstm_cell_bwd(_p(acts), _p(c_t), _p(c_prev), _p(dh), _p(dh_slabs), nslabs, slab_stride,
                                            _p(dc), _p(seq_len), t, B, H, _p(dgates), _p(dc_prev), _p(dh_carry),
                                            _stream()), "ds_lstm_cell_bwd")


def lstm_seq_supported(B, H):
    return bool(_lib.load().ds_lstm_seq_supported(B, H))


def lstm_seq_workspace(B, H):
    return int(_lib.load().ds_lstm_seq_workspace(B, H))


def lstm_seq_fwd(gates, wh_ptr, ldw, h, c, seq_len, T, B, H, forget_bias, ws, rows=1):
    """rows: row groups per workgroup (1, 2, 4, 8) -- scheduling only.  `ws` is zeroed once by its owner."""
    _lib.check(_lib.load().ds_lstm_seq_fwd(_p(gates), wh_ptr, ldw, _p(h), _p(c), _p(seq_len), T, B, H, forget_bias,
                                           int(rows), _p(ws), ws.numel() * ws.element_size(), _stream()),
               "ds_lstm_seq_fwd")


def lstm_seq_bwd(acts, wh_ptr, ldw, c, dh_last, ld_dh, seq_len, T, B, H, dgates, ws, rows=1):
    _lib.check(_lib.load().ds_lstm_seq_bwd(_p(acts), wh_ptr, ldw, _p(c), _p(dh_last), ld_dh, _p(seq_len), T, B, H,
                                           _p(dgates), int(rows), _p(ws), ws.numel() * ws.element_size(), _stream()),
               "ds_lstm_seq_bwd")


def seq_sort_desc(seq_len, B, T, perm, len_sorted):
    """perm [B] int32, len_sorted [B] int64: the batch in descending order of length (ties by index), on the device."""
    _lib.check(_lib.load().ds_seq_sort_desc(_p(seq_len), B, T, _p(perm), _p(len_sorted), _stream()), "ds_seq_sort_desc")


def permute_rows(src, dst, perm, rows, cols, gather=True):
    """gather: dst[j] = src[perm[j]]; scatter (gather=False): dst[perm[j]] = src[j].  fp32 or int64 rows."""
    assert src.element_size() == dst.element_size() and src.element_size() in (4, 8)
    _lib.check(_lib.load().ds_permute_rows(_p(src), src.stride(0), _p(dst), dst.stride(0), _p(perm), rows, cols, src.element_size(),
                                           int(bool(gather)), _stream()), "ds_permute_rows")


def lstm_seq_status(ws, B):
    """0 = ok; call after a synchronise (it copies two words to the host).  Raises on a hand-off timeout of any
    forward (bit 0) or backward (bit 1) launch since the last read: the error words are sticky until reported, then cleared."""
    rc = _lib.load().ds_lstm_seq_status(_p(ws), B)
    if rc != 0:
        which = " and ".join(n for b, n in ((1, "forward"), (2, "backward")) if rc > 0 and rc & b) or "status read"
        raise RuntimeError("ds_lstm_seq: a workgroup hand-off of the %s launch timed out (status %d): the LSTM results "
                           "of this step are invalid (a workgroup of a row group never became resident)" % (which, rc))
    return rc


def softmax_ce(logits, labels, B, C_, grad_scale, grad_scale_dev, loss, dlogits):
    _lib.check(_lib.load().ds_softmax_ce(_p(logits), _p(labels), B, C_, grad_scale, _p(grad_scale_dev), _p(loss),
                                         _p(dlogits), _stream()), "ds_softmax_ce")


def softmax_ce_opts(ce, logits, labels, B, C_, grad_scale, grad_scale_dev, loss, dlogits):
    """softmax_ce with label smoothing and per-class weights (ce: a ce_desc; None: softmax_ce's bits)."""
    _lib.check(_lib.load().ds_softmax_ce_opts(None if ce is None else C.byref(ce), _p(logits), _p(labels), B, C_, grad_scale,
                                              _p(grad_scale_dev), _p(loss), _p(dlogits), _stream()), "ds_softmax_ce_opts")


def adam_tf(theta, g, m, v, n, n_wd, wd, grad_scale, lr_t, b1, b2, eps, lr_t_dev=None):
    _lib.check(_lib.load().ds_adam_tf(_p(theta), _p(g), _p(m), _p(v), n, n_wd, wd, grad_scale, lr_t, _p(lr_t_dev),
                                      b1, b2, eps, _stream()), "ds_adam_tf")


CLIP_NONE, CLIP_PER_VARIABLE, CLIP_GLOBAL = 0, 1, 2


def grad_norms(theta, g, n, n_wd, wd, grad_scale, segments, chunks, mode, clip, skip_nonfinite, partials, sumsq, factors,
               flags):
    """Per-variable and global sums of squares of the effective gradient, the clipping factors and the skip flag
    (ds_grad_norms): segments int64 [nseg, 8], chunks int64 [nchunks, 4] (ParamStore.clip_tables), partials float64 [nchunks],
    sumsq float64 [nseg + 1], factors float32 [nseg + 1], flags int32 [4].  Two launches, nothing is read back."""
    nseg, nchunks = segments.shape[0], chunks.shape[0]
    assert partials.dtype == torch.float64 and partials.numel() >= nchunks
    assert sumsq.dtype == torch.float64 and sumsq.numel() >= nseg + 1
    assert factors.dtype == torch.float32 and factors.numel() >= nseg + 1
    assert flags.dtype == torch.int32 and flags.numel() >= 4
    assert segments.dtype == torch.int64 and chunks.dtype == torch.int64 and segments.shape[1] == 8 and chunks.shape[1] == 4
    _lib.check(_lib.load().ds_grad_norms(_p(theta), _p(g), n, n_wd, wd, grad_scale, _p(segments), nseg, _p(chunks), nchunks,
                                         mode, float(clip), int(bool(skip_nonfinite)), _p(partials), _p(sumsq), _p(factors),
                                         _p(flags), _stream()), "ds_grad_norms")


def adam_tf_clipped(theta, g, m, v, n, n_wd, wd, grad_scale, lr_t, b1, b2, eps, segments, chunks, factors, flags,
                    lr_t_dev=None):
    """ds_adam_tf on g_eff * factors[segment], skipped as a whole when flags[1] is set (ds_adam_tf_clipped)."""
    nseg, nchunks = segments.shape[0], chunks.shape[0]
    assert factors.dtype == torch.float32 and factors.numel() >= nseg + 1 and flags.dtype == torch.int32 and flags.numel() >= 4
    assert segments.dtype == torch.int64 and chunks.dtype == torch.int64 and segments.shape[1] == 8 and chunks.shape[1] == 4
    _lib.check(_lib.load().ds_adam_tf_clipped(_p(theta), _p(g), _p(m), _p(v), n, n_wd, wd, grad_scale, lr_t, _p(lr_t_dev),
                                              b1, b2, eps, _p(segments), nseg, _p(chunks), nchunks, _p(factors), _p(flags),
                                              _stream()), "ds_adam_tf_clipped")


def adam_tf_ema(theta, g, m, v, shadow, n, n_wd, wd, grad_scale, lr_t, ema_rate, b1, b2, eps, lr_t_dev=None,
                ema_rate_dev=None):
    """ds_adam_tf plus shadow -= (shadow - theta_new) * ema_rate in the same pass (ds_adam_tf_ema)."""
    assert shadow.dtype == torch.float32 and shadow.numel() >= n
    _lib.check(_lib.load().ds_adam_tf_ema(_p(theta), _p(g), _p(m), _p(v), _p(shadow), n, n_wd, wd, grad_scale, lr_t,
                                          _p(lr_t_dev), ema_rate, _p(ema_rate_dev), b1, b2, eps, _stream()), "ds_adam_tf_ema")


def adam_tf_clipped_ema(theta, g, m, v, shadow, n, n_wd, wd, grad_scale, lr_t, ema_rate, b1, b2, eps, segments, chunks,
                        factors, flags, lr_t_dev=None, ema_rate_dev=None):
    """ds_adam_tf_clipped plus the shadow update of ds_adam_tf_ema; a skipped step leaves the shadows alone too."""
    nseg, nchunks = segments.shape[0], chunks.shape[0]
    assert shadow.dtype == torch.float32 and shadow.numel() >= n
    assert factors.dtype == torch.float32 and factors.numel() >= nseg + 1 and flags.dtype == torch.int32 and flags.numel() >= 4
    assert segments.dtype == torch.int64 and chunks.dtype == torch.int64 and segments.shape[1] == 8 and chunks.shape[1] == 4
    _lib.check(_lib.load().ds_adam_tf_clipped_ema(_p(theta), _p(g), _p(m), _p(v), _p(shadow), n, n_wd, wd, grad_scale, lr_t,
                                                  _p(lr_t_dev), ema_rate, _p(ema_rate_dev), b1, b2, eps, _p(segments), nseg,
                                                  _p(chunks), nchunks, _p(factors), _p(flags), _stream()),
               "ds_adam_tf_clipped_ema")


OPT_ADAM, OPT_SGD, OPT_MOMENTUM, OPT_RMSPROP = 0, 1, 2, 3
OPT_KINDS = {"adam": OPT_ADAM, "sgd": OPT_SGD, "momentum": OPT_MOMENTUM, "rmsprop": OPT_RMSPROP}


def opt_step(kind, theta, g, slot0, slot1, n, n_wd, wd, grad_scale, lr, b1=0.0, b2=0.0, eps=0.0, momentum=0.0, rho=0.0,
             lr_dev=None, shadow=None, ema_rate=0.0, ema_rate_dev=None, segments=None, chunks=None, factors=None, flags=None):
    """One optimiser step of `kind` (OPT_*) over a flat buffer (ds_opt_step): lr is Adam's lr_t for OPT_ADAM and the learning
    rate otherwise; slot0 / slot1 are Adam's m / v, momentum's accumulator / nothing, RMSProp's mom / ms (sgd reads neither).
    shadow: the moving-average update of adam_tf_ema in the same pass.  segments, chunks, factors, flags (all four or none):
    the clipped pass behind grad_norms, skipped as a whole when flags[1] is set."""
    d = _lib.OptDesc()
    d.kind, d.lr, d.lr_dev = int(kind), lr, _p(lr_dev)
    d.b1, d.b2, d.eps, d.momentum, d.rho = b1, b2, eps, momentum, rho
    if shadow is not None:
        assert shadow.dtype == torch.float32 and shadow.numel() >= n
    d.shadow, d.ema_rate, d.ema_rate_dev = _p(shadow), ema_rate, _p(ema_rate_dev)
    if segments is not None or chunks is not None:
        nseg, nchunks = segments.shape[0], chunks.shape[0]
        assert segments.dtype == torch.int64 and chunks.dtype == torch.int64 and segments.shape[1] == 8 and chunks.shape[1] == 4
        assert factors is None or (factors.dtype == torch.float32 and factors.numel() >= nseg + 1)
        assert flags is None or (flags.dtype == torch.int32 and flags.numel() >= 4)
        d.segments, d.chunks, d.nseg, d.nchunks = _p(segments), _p(chunks), nseg, nchunks
    d.factors, d.flags = _p(factors), _p(flags)
    _lib.check(_lib.load().ds_opt_step(C.byref(d), _p(theta), _p(g), _p(slot0), _p(slot1), n, n_wd, wd, grad_scale, _stream()),
               "ds_opt_step")


def grad_accumulate(acc, g, n, mode):
    """Clone-gradient accumulation over the first n floats of two flat buffers: mode 0 acc = g, 1 acc = acc + g,
    2 g = acc + g (the running sum is the left operand; n % 4 == 0, 16-byte aligned)."""
    _lib.check(_lib.load().ds_grad_accumulate(_p(acc), _p(g), n, mode, _stream()), "ds_grad_accumulate")


def sumsq(x, n, scratch, out):
    _lib.check(_lib.load().ds_sumsq(_p(x), n, _p(scratch), _p(out), _stream()), "ds_sumsq")


def colsum(x, M, C_, ld, scratch, out):
    _lib.check(_lib.load().ds_colsum(_p(x), M, C_, ld, _p(scratch), _p(out), _stream()), "ds_colsum")


def copy2d(src, lds, dst, ldd, rows, cols):
    _lib.check(_lib.load().ds_copy2d(_p(src), lds, _p(dst), ldd, rows, cols, _stream()), "ds_copy2d")


def pad_channels(src, cs, dst, cd, pixels):
    _lib.check(_lib.load().ds_pad_channels(_p(src), cs, _p(dst), cd, pixels, _stream()), "ds_pad_channels")


def fill(dst, n, value):
    _lib.check(_lib.load().ds_fill(_p(dst), n, value, _stream()), "ds_fill")


# ---- streaming evaluation metrics (ds_eval_metrics_update) ------------------------------------------------------------------
def eval_metrics_workspace(B, C_):
    """Bytes of scratch ds_eval_metrics_update needs for a [B, C_] batch (host only)."""
    n = _lib.load().ds_eval_metrics_workspace(B, C_)
    _lib.check(min(n, 0), "ds_eval_metrics_workspace")
    return n


def eval_metrics_update(logits, labels, counts, loss_sum, scratch):
    """Add the batch (fp32 logits [B, C], unit column stride; int64 labels [B]) to counts (int64 [C*C + C + 4]) and loss_sum
    (float64 [1]) on the current stream: include/ds_kernels.h has the layout.  Nothing is read back."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("eval_metrics_update: logits must be fp32 [B, C] with unit column stride")
    B, C_ = logits.shape
    if labels.dtype != torch.int64 or labels.shape != (B,) or not labels.is_contiguous():
        raise ValueError("eval_metrics_update: labels must be contiguous int64 [B]")
    if counts.dtype != torch.int64 or counts.numel() != C_ * C_ + C_ + 4 or not counts.is_contiguous():
        raise ValueError("eval_metrics_update: counts must be contiguous int64 [C*C + C + 4]")
    if loss_sum.dtype != torch.float64 or loss_sum.numel() != 1:
        raise ValueError("eval_metrics_update: loss_sum must be one float64")
    need = eval_metrics_workspace(B, C_)
    if scratch.numel() * scratch.element_size() < need or not scratch.is_contiguous():
        raise ValueError("eval_metrics_update: scratch is smaller than eval_metrics_workspace(B, C) = %d bytes" % need)
    _lib.check(_lib.load().ds_eval_metrics_update(_p(logits), logits.stride(0), _p(labels), B, C_, _p(counts), _p(loss_sum),
                                                  _p(scratch), _stream()), "ds_eval_metrics_update")


# ---- eval-time image preprocessing (ds_preprocess_eval) ---------------------------------------------------------------------
def preprocess_desc_dtype():
    """NumPy view of ds_preprocess_desc (24 bytes): one record per image of a ragged uint8 batch."""
    import numpy as np
    return np.dtype([("offset", np.int64), ("height", np.int32), ("width", np.int32),
                     ("scale_y", np.float32), ("scale_x", np.float32)], align=True)


def preprocess_train_desc_dtype():
    """NumPy view of ds_preprocess_train_desc (40 bytes): the eval record + brightness delta, saturation factor, flags
    (_lib.DS_PREPROCESS_FLIP | _lib.DS_PREPROCESS_SATURATION_FIRST) and a reserved word that stays 0."""
    import numpy as np
    return np.dtype([("offset", np.int64), ("height", np.int32), ("width", np.int32),
                     ("scale_y", np.float32), ("scale_x", np.float32), ("delta", np.float32), ("factor", np.float32),
                     ("flags", np.uint32), ("reserved", np.uint32)], align=True)


def _check_descs(desc, nbytes, dtype, what):
    import numpy as np
    desc = np.asarray(desc)
    if desc.dtype != dtype or desc.ndim != 1 or desc.size == 0:
        raise ValueError("%s: descriptors must be a non-empty 1-D array of ops.%s()"
                         % (what, "preprocess_train_desc_dtype" if what == "preprocess_train" else "preprocess_desc_dtype"))
    h, w, off = desc["height"].astype(np.int64), desc["width"].astype(np.int64), desc["offset"]
    bad = (h < 1) | (w < 1) | (off < 0) | (off + h * w * 3 > int(nbytes))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError("%s: descriptor %d (offset %d, %d x %d pixels) does not fit the byte buffer of %d bytes"
                         % (what, i, int(off[i]), int(h[i]), int(w[i]), int(nbytes)))
    if not (np.isfinite(desc["scale_y"]).all() and np.isfinite(desc["scale_x"]).all()
            and (desc["scale_y"] > 0).all() and (desc["scale_x"] > 0).all()):
        raise ValueError("%s: scales must be finite and positive" % what)
    return desc


def check_preprocess_descs(desc, nbytes):
    """Every image of the descriptor table lies inside a byte buffer of `nbytes` bytes (the kernel cannot check): raises
    ValueError before anything is launched."""
    _check_descs(desc, nbytes, preprocess_desc_dtype(), "preprocess_eval")


def check_preprocess_train_descs(desc, nbytes):
    """check_preprocess_descs for ds_preprocess_train_desc records; additionally delta and factor are finite, factor >= 0,
    no unknown flag bit is set and the reserved word is 0."""
    import numpy as np
    desc = _check_descs(desc, nbytes, preprocess_train_desc_dtype(), "preprocess_train")
    if not (np.isfinite(desc["delta"]).all() and np.isfinite(desc["factor"]).all() and (desc["factor"] >= 0).all()):
        raise ValueError("preprocess_train: delta and factor must be finite and factor >= 0")
    known = _lib.DS_PREPROCESS_FLIP | _lib.DS_PREPROCESS_SATURATION_FIRST
    if (desc["flags"] & ~np.uint32(known)).any() or desc["reserved"].any():
        raise ValueError("preprocess_train: unknown flag bits (or a non-zero reserved word)")


_preprocess_lut = {}


def preprocess_lut(device):
    """The 256-entry uint8 -> [0, 1] table of convert_image_dtype, np.arange(256, f32) / f32(255), on `device` (cached)."""
    import numpy as np
    dev = torch.device(device)
    key = torch.cuda.current_device() if dev.index is None else dev.index
    if key not in _preprocess_lut:
        lut = np.arange(256, dtype=np.float32) / np.float32(255)
        _preprocess_lut[key] = torch.from_numpy(lut).to(torch.device("cuda", key))
    return _preprocess_lut[key]


def _preprocess(what, check, itemsize, image_bytes, desc, out_h, out_w, desc_dev, out):
    import numpy as np
    if not image_bytes.is_cuda:
        raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
    if image_bytes.dtype != torch.uint8 or not image_bytes.is_contiguous():
        raise ValueError("%s: image_bytes must be a contiguous uint8 tensor" % what)
    if out_h < 1 or out_w < 1:
        raise ValueError("%s: out_h and out_w must be positive" % what)
    check(desc, image_bytes.numel())
    B = int(np.asarray(desc).size)
    if desc_dev is None:
        desc_dev = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(image_bytes.device)
    if desc_dev.numel() * desc_dev.element_size() < B * itemsize or not desc_dev.is_contiguous():
        raise ValueError("%s: desc_dev is smaller than the descriptor table" % what)
    if out is None:
        out = torch.empty((B, out_h, out_w, 3), dtype=torch.float32, device=image_bytes.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * out_h * out_w * 3:
        raise ValueError("%s: out must be a contiguous fp32 [B, out_h, out_w, 3] tensor" % what)
    fn = getattr(_lib.load(), "ds_" + what)
    _lib.check(fn(_p(image_bytes), image_bytes.numel(), _p(desc_dev), B, _p(preprocess_lut(image_bytes.device)),
                  _p(out), out_h, out_w, _stream()), "ds_" + what)
    return out


def preprocess_eval(image_bytes, desc, out_h, out_w, desc_dev=None, out=None):
    """preprocess_for_eval of a ragged batch in one launch.  image_bytes: device uint8 tensor holding the centrally cropped
    HWC images back to back; desc: HOST array of ops.preprocess_desc_dtype() records (checked against the buffer's size
    here, before the launch); desc_dev: the same table already on the device (uploaded here when None); out: fp32
    [B, out_h, out_w, 3] (allocated when None).  Returns out."""
    return _preprocess("preprocess_eval", check_preprocess_descs, preprocess_desc_dtype().itemsize, image_bytes, desc,
                       out_h, out_w, desc_dev, out)


def preprocess_train(image_bytes, desc, out_h, out_w, desc_dev=None, out=None):
    """preprocess_for_train of a ragged batch in one launch (ds_preprocess_train): as preprocess_eval, with the sampled
    crops in image_bytes and ops.preprocess_train_desc_dtype() records, which also carry each image's flip, colour order,
    brightness delta and saturation factor."""
    return _preprocess("preprocess_train", check_preprocess_train_descs, preprocess_train_desc_dtype().itemsize,
                       image_bytes, desc, out_h, out_w, desc_dev, out)


# ---- baseline JPEG decode: host entropy decoder + ds_jpeg_reconstruct ----------------------------------------------------------
JPEG_TEXT_CAPACITY = 50             # datasets.convert_to_dataset._POST_SIZE: the ids one record may carry


def jpeg_desc_dtype():
    """NumPy view of ds_jpeg_desc (240 bytes): one record per image of a ragged ds_jpeg_reconstruct launch."""
    import numpy as np
    return np.dtype([("coef_offset", np.int64), ("out_offset", np.int64), ("width", np.int32), ("height", np.int32),
                     ("sampling", np.int32), ("y0", np.int32), ("x0", np.int32), ("crop_h", np.int32), ("crop_w", np.int32),
                     ("reserved", np.int32), ("quant", np.uint8, (3, 64))], align=True)


def jpeg_blocks(height, width, sampling):
    """8 x 8 blocks of the padded (whole-MCU) grids of an image, all components: its coefficient storage is 64 int16 each."""
    if sampling == _lib.DS_JPEG_GREY:
        return -(-width // 8) * -(-height // 8)
    h, v = (2 if sampling in (_lib.DS_JPEG_422, _lib.DS_JPEG_420) else 1), (2 if sampling == _lib.DS_JPEG_420 else 1)
    return -(-width // (8 * h)) * -(-height // (8 * v)) * (h * v + 2)


def check_jpeg_descs(desc, ncoef, nbytes):
    """Every image of the table has a known sampling class, a crop inside the image, its coefficients inside a buffer of
    `ncoef` int16 (offset a multiple of 8) and its crop inside a byte buffer of `nbytes` bytes (offset a multiple of 4), and
    no two crops overlap: raises ValueError before anything is launched (the kernels cannot report a bad descriptor)."""
    import numpy as np
    desc = np.asarray(desc)
    if desc.dtype != jpeg_desc_dtype() or desc.ndim != 1 or desc.size == 0:
        raise ValueError("jpeg_reconstruct: descriptors must be a non-empty 1-D array of ops.jpeg_desc_dtype()")
    i64 = lambda k: desc[k].astype(np.int64)
    w, h, s = i64("width"), i64("height"), i64("sampling")
    if ((s < 0) | (s > 3) | (w < 1) | (h < 1) | (w > 65535) | (h > 65535)).any() or desc["reserved"].any():
        raise ValueError("jpeg_reconstruct: bad image size or sampling class")
    y0, x0, ch, cw = i64("y0"), i64("x0"), i64("crop_h"), i64("crop_w")
    if ((y0 < 0) | (x0 < 0) | (ch < 1) | (cw < 1) | (y0 + ch > h) | (x0 + cw > w)).any():
        raise ValueError("jpeg_reconstruct: a crop box leaves its image")
    hs, vs = np.where((s == 1) | (s == 2), 2, 1), np.where(s == 2, 2, 1)         # jpeg_blocks, for the whole table at once
    need = -(-w // (8 * hs)) * -(-h // (8 * vs)) * np.where(s == 3, 1, hs * vs + 2) * 64
    co, oo = desc["coef_offset"], desc["out_offset"]
    if ((co < 0) | (co % 8 != 0) | (co + need > int(ncoef))).any():
        raise ValueError("jpeg_reconstruct: coefficients outside the buffer of %d int16 (or an offset that is no multiple of 8)" % int(ncoef))
    end = oo + ch * cw * 3
    if ((oo < 0) | (oo % 4 != 0) | (end > int(nbytes))).any():
        raise ValueError("jpeg_reconstruct: a crop outside the byte buffer of %d bytes (or an offset that is no multiple of 4)" % int(nbytes))
    order = np.argsort(oo, kind="stable")
    if (end[order][:-1] > oo[order][1:]).any():
        raise ValueError("jpeg_reconstruct: two crops overlap in the byte buffer")
    order = np.argsort(co, kind="stable")
    if ((co + need)[order][:-1] > co[order][1:]).any():
        raise ValueError("jpeg_reconstruct: two images share coefficient storage (their planes share the scratch)")
    return desc


def _host_ptr(a):
    return C.c_void_p(a.ctypes.data)


def jpeg_probe(data):
    """ds_jpeg_probe of a bytes object: the _lib.JpegInfo of a supported stream, None otherwise."""
    info = _lib.JpegInfo()
    rc = _lib.load().ds_jpeg_probe(C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(info))
    if rc < 0:
        raise ValueError("ds_jpeg_probe: bad argument")
    return info if rc == 0 and info.supported else None


def jpeg_entropy_decode(data, info):
    """ds_jpeg_entropy_decode: int16 coefficients (natural order, block raster over the padded grids, component after
    component) of a stream ds_jpeg_probe supports; None when the entropy-coded data turn out to be outside the set."""
    import numpy as np
    coef = np.empty(int(info.coef_count), np.int16)
    rc = _lib.load().ds_jpeg_entropy_decode(C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(info), _host_ptr(coef), coef.size)
    if rc < 0 or rc == _lib.DS_JPEG_MORE:
        raise ValueError("ds_jpeg_entropy_decode: bad argument (%d)" % rc)
    return coef if rc == 0 else None


def jpeg_quant(info):
    """The [3, 64] uint8 quantisation tables of a JpegInfo (natural order), as a descriptor's `quant` field takes them."""
    import numpy as np
    return np.frombuffer(bytes(info.quant), np.uint8).reshape(3, 64)


def example_parse(rec):
    """ds_example_parse of one TFRecord payload: (image offset, image length, text int64[50], seq_len, label, post_id,
    day), or None when the compiled reader does not take the payload (the Python parser decides then)."""
    import numpy as np
    text = np.zeros(JPEG_TEXT_CAPACITY, np.int64)
    f = _lib.ExampleFields()
    rc = _lib.load().ds_example_parse(C.cast(C.c_char_p(rec), C.c_void_p), len(rec), _host_ptr(text), text.size, C.byref(f))
    if rc < 0:
        raise ValueError("ds_example_parse: bad argument")
    if rc != 0:
        return None
    return f.image_offset, f.image_length, text, f.seq_len, f.label, f.post_id, f.day


def jpeg_record_decode(rec, coef):
    """One call per record (the GIL is released for its duration): parse the payload, probe the JPEG and Huffman-decode it
    into `coef` (a C-contiguous int16 array) when it fits.  Returns None when the payload is not taken, otherwise
    (status, info, fields tuple as example_parse) with status DS_OK (coef[:info.coef_count] holds the image),
    _lib.DS_JPEG_UNSUPPORTED or _lib.DS_JPEG_MORE (info.coef_count int16 are needed)."""
    import numpy as np
    text = np.zeros(JPEG_TEXT_CAPACITY, np.int64)
    f, info, status = _lib.ExampleFields(), _lib.JpegInfo(), C.c_int32(0)
    rc = _lib.load().ds_jpeg_record_decode(C.cast(C.c_char_p(rec), C.c_void_p), len(rec), _host_ptr(text), text.size, C.byref(f),
                                           C.byref(info), _host_ptr(coef) if coef.size else None, coef.size, C.byref(status))
    if rc < 0:
        raise ValueError("ds_jpeg_record_decode: bad argument")
    if rc != 0:
        return None
    return status.value, info, (f.image_offset, f.image_length, text, f.seq_len, f.label, f.post_id, f.day)


def jpeg_reconstruct_host(coef, desc, out_bytes):
    """ds_jpeg_reconstruct_host on NumPy arrays: fills the crops of `desc` in out_bytes (uint8) from coef (int16)."""
    import numpy as np
    desc = check_jpeg_descs(desc, coef.size, out_bytes.size)
    if coef.dtype != np.int16 or out_bytes.dtype != np.uint8 or not coef.flags.c_contiguous or not out_bytes.flags.c_contiguous:
        raise ValueError("jpeg_reconstruct_host: coef int16 and out_bytes uint8, both contiguous")
    desc = np.ascontiguousarray(desc)
    rc = _lib.load().ds_jpeg_reconstruct_host(_host_ptr(coef), coef.size, _host_ptr(desc), desc.size, _host_ptr(out_bytes), out_bytes.size)
    if rc != 0:
        raise ValueError("ds_jpeg_reconstruct_host: bad descriptor (%d)" % rc)
    return out_bytes


def jpeg_reconstruct(coef, desc, out_bytes, scratch=None, desc_dev=None):
    """ds_jpeg_reconstruct: coef (device int16), desc (HOST array of ops.jpeg_desc_dtype(), checked here), out_bytes (device
    uint8, written in place: only the crops' bytes), scratch (device uint8, >= coef.numel() bytes; allocated when None),
    desc_dev (the table already on the device; uploaded here when None).  Returns out_bytes."""
    import numpy as np
    if not (coef.is_cuda and out_bytes.is_cuda):
        raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
    if coef.dtype != torch.int16 or out_bytes.dtype != torch.uint8 or not coef.is_contiguous() or not out_bytes.is_contiguous():
        raise ValueError("jpeg_reconstruct: coef must be a contiguous int16 tensor and out_bytes a contiguous uint8 tensor")
    desc = check_jpeg_descs(desc, coef.numel(), out_bytes.numel())
    B = int(desc.size)
    if desc_dev is None:
        desc_dev = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(coef.device)
    if desc_dev.numel() * desc_dev.element_size() < B * jpeg_desc_dtype().itemsize or not desc_dev.is_contiguous():
        raise ValueError("jpeg_reconstruct: desc_dev is smaller than the descriptor table")
    if scratch is None:
        scratch = torch.empty(coef.numel(), dtype=torch.uint8, device=coef.device)
    if scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < coef.numel():
        raise ValueError("jpeg_reconstruct: scratch must be a contiguous uint8 tensor of at least coef.numel() bytes")
    _lib.check(_lib.load().ds_jpeg_reconstruct(_p(coef), coef.numel(), _p(desc_dev), B, _p(out_bytes), out_bytes.numel(),
                                               _p(scratch), scratch.numel(), _stream()), "ds_jpeg_reconstruct")
    return out_bytes


# ---- restart-segmented JPEGs: scan description, lossless restart transcoder, the Huffman decode on the device ------------------
def jpeg_huff_dtype():
    """NumPy view of ds_jpeg_huff (272 bytes): a Huffman table in its DHT form."""
    import numpy as np
    return np.dtype([("counts", np.uint8, (16,)), ("values", np.uint8, (256,))])


def jpeg_scan_desc_dtype():
    """NumPy view of ds_jpeg_scan_desc (1856 bytes): one record per image of a ds_jpeg_entropy_decode_device launch."""
    import numpy as np
    return np.dtype([("coef_offset", np.int64), ("width", np.int32), ("height", np.int32), ("sampling", np.int32),
                     ("first_segment", np.int32), ("segments", np.int32), ("reserved", np.int32), ("quant", np.uint8, (3, 64)),
                     ("dc", jpeg_huff_dtype(), (3,)), ("ac", jpeg_huff_dtype(), (3,))], align=True)


def jpeg_segment_dtype():
    """NumPy view of ds_jpeg_segment (24 bytes): one record per restart segment."""
    import numpy as np
    return np.dtype([("begin", np.int64), ("end", np.int64), ("first_mcu", np.int32), ("mcus", np.int32)], align=True)


def jpeg_mcus(height, width, sampling):
    """(MCUs per row, MCU rows) of an image."""
    h, v = (2 if sampling in (_lib.DS_JPEG_422, _lib.DS_JPEG_420) else 1), (2 if sampling == _lib.DS_JPEG_420 else 1)
    return -(-width // (8 * h)), -(-height // (8 * v))


def jpeg_scan(data):
    """ds_jpeg_scan of a bytes object: (_lib.JpegInfo, _lib.JpegScanInfo, int64 cut positions) of a supported stream --
    markers and the walk over the entropy-coded bytes only, nothing is decoded -- or None where ds_jpeg_probe says
    unsupported."""
    import numpy as np
    info, scan = _lib.JpegInfo(), _lib.JpegScanInfo()
    cuts = np.empty(64, np.int64)
    for _ in range(2):
        rc = _lib.load().ds_jpeg_scan(C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(info), C.byref(scan), _host_ptr(cuts), cuts.size)
        if rc != _lib.DS_JPEG_MORE:
            break
        cuts = np.empty(int(scan.cut_count), np.int64)
    if rc < 0:
        raise ValueError("ds_jpeg_scan: bad argument")
    return (info, scan, cuts[:int(scan.cut_count)]) if rc == 0 else None


def jpeg_record_scan(rec, cuts):
    """One call per record (the GIL is released for its duration): parse the payload and describe the JPEG's scan; `cuts`
    is a C-contiguous int64 array for the cut positions.  Returns None when the payload is not taken, otherwise (status,
    info, scan, fields tuple as example_parse) with status DS_OK (cuts[:scan.cut_count] are valid), _lib.DS_JPEG_UNSUPPORTED
    or _lib.DS_JPEG_MORE (scan.cut_count entries are needed).  Positions count from the image's first byte."""
    import numpy as np
    text = np.zeros(JPEG_TEXT_CAPACITY, np.int64)
    f, info, scan, status = _lib.ExampleFields(), _lib.JpegInfo(), _lib.JpegScanInfo(), C.c_int32(0)
    rc = _lib.load().ds_jpeg_record_scan(C.cast(C.c_char_p(rec), C.c_void_p), len(rec), _host_ptr(text), text.size, C.byref(f),
                                         C.byref(info), C.byref(scan), _host_ptr(cuts) if cuts.size else None, cuts.size,
                                         C.byref(status))
    if rc < 0:
        raise ValueError("ds_jpeg_record_scan: bad argument")
    if rc != 0:
        return None
    return status.value, info, scan, (f.image_offset, f.image_length, text, f.seq_len, f.label, f.post_id, f.day)


def jpeg_restart_transcode(data, interval_mcus=0):
    """ds_jpeg_restart_transcode: the stream re-encoded losslessly with a restart interval of `interval_mcus` MCUs (0 = one
    MCU row) as bytes, or None when the stream is outside the supported set (the caller keeps the original)."""
    import numpy as np
    out = np.empty(len(data) + len(data) // 4 + 4096, np.uint8)
    n = C.c_int64(0)
    for _ in range(2):
        rc = _lib.load().ds_jpeg_restart_transcode(C.cast(C.c_char_p(data), C.c_void_p), len(data), int(interval_mcus), _host_ptr(out),
                                                   out.size, C.byref(n))
        if rc != _lib.DS_JPEG_MORE:
            break
        out = np.empty(n.value, np.uint8)
    if rc < 0:
        raise ValueError("ds_jpeg_restart_transcode: bad argument (interval_mcus must be 0 .. 65535)")
    return out[:n.value].tobytes() if rc == 0 else None


def fill_jpeg_scan_tables(streams, coef_offsets, scan, images, segs):
    """Lay the entropy-coded bytes of `streams` -- [(encoded bytes, info, scan info, cuts)] as jpeg_scan returns them --
    back to back into `scan` (uint8) and describe them: images[i] (ops.jpeg_scan_desc_dtype(), coefficient storage at
    coef_offsets[i]) and one segs record (ops.jpeg_segment_dtype()) per restart segment.  The arrays must be large enough.
    Returns (scan bytes used, segments used)."""
    import numpy as np
    raw = images.view(np.uint8).reshape(images.size, -1)
    pos = nseg = 0
    for i, (data, info, si, cuts) in enumerate(streams):
        begin, end, n = int(si.scan_begin), int(cuts[-1]), int(cuts.size)
        scan[pos:pos + end - begin] = np.frombuffer(data, np.uint8, end - begin, begin)
        images[i] = (coef_offsets[i], info.width, info.height, info.sampling, nseg, n, 0, 0, 0, 0)
        raw[i, 32:224] = np.frombuffer(info.quant, np.uint8)
        raw[i, 224:] = np.frombuffer(si, np.uint8, 6 * 272, 16)            # dc[3], ac[3]: the same layout in both structs
        mw, mh = jpeg_mcus(info.height, info.width, info.sampling)
        interval = info.restart_interval or mw * mh
        s = segs[nseg:nseg + n]
        s["end"] = cuts + (pos - begin)
        s["begin"][0] = pos
        s["begin"][1:] = s["end"][:-1] + 2
        first = np.arange(n, dtype=np.int64) * interval
        s["first_mcu"] = first
        s["mcus"] = np.minimum(interval, mw * mh - first)
        pos += end - begin
        nseg += n
    return pos, nseg


def make_jpeg_scan_tables(streams, coef_offsets=None):
    """fill_jpeg_scan_tables into new arrays: (scan uint8, images, segs, coefficient count); coefficient storage back to
    back (starts rounded up to 8 int16) when coef_offsets is None."""
    import numpy as np
    if coef_offsets is None:
        coef_offsets, cpos = [], 0
        for _, info, _, _ in streams:
            coef_offsets.append(cpos)
            cpos = -(-(cpos + int(info.coef_count)) // 8) * 8
    ncoef = max(o + int(st[1].coef_count) for o, st in zip(coef_offsets, streams))
    scan = np.zeros(max(1, sum(int(c[-1]) - int(si.scan_begin) for _, _, si, c in streams)), np.uint8)
    images = np.zeros(len(streams), jpeg_scan_desc_dtype())
    segs = np.zeros(sum(c.size for _, _, _, c in streams), jpeg_segment_dtype())
    fill_jpeg_scan_tables(streams, coef_offsets, scan, images, segs)
    return scan, images, segs, ncoef


def check_jpeg_scan_descs(images, segs, nscan, ncoef):
    """Every image of the table has a known sampling class, its coefficients inside a buffer of `ncoef` int16 (offset a
    multiple of 8, no two images on the same storage) and its segments inside `segs`; every segment has its bytes inside a
    scan buffer of `nscan` bytes, and the segments of an image continue each other from MCU 0 to the image's last: raises
    ValueError before anything is launched.  (What the bytes and the Huffman tables hold is the kernel's to judge: it
    reports that per image.)"""
    import numpy as np
    images, segs = np.asarray(images), np.asarray(segs)
    if images.dtype != jpeg_scan_desc_dtype() or images.ndim != 1 or images.size == 0:
        raise ValueError("jpeg_entropy_decode: images must be a non-empty 1-D array of ops.jpeg_scan_desc_dtype()")
    if segs.dtype != jpeg_segment_dtype() or segs.ndim != 1 or segs.size == 0:
        raise ValueError("jpeg_entropy_decode: segs must be a non-empty 1-D array of ops.jpeg_segment_dtype()")
    i64 = lambda a, k: a[k].astype(np.int64)
    w, h, s = i64(images, "width"), i64(images, "height"), i64(images, "sampling")
    if ((s < 0) | (s > 3) | (w < 1) | (h < 1) | (w > 65535) | (h > 65535)).any() or images["reserved"].any():
        raise ValueError("jpeg_entropy_decode: bad image size or sampling class")
    hs, vs = np.where((s == 1) | (s == 2), 2, 1), np.where(s == 2, 2, 1)
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    need = mcus * np.where(s == 3, 1, hs * vs + 2) * 64
    co = images["coef_offset"]
    if ((co < 0) | (co % 8 != 0) | (co + need > int(ncoef))).any():
        raise ValueError("jpeg_entropy_decode: coefficients outside the buffer of %d int16 (or an offset that is no multiple of 8)" % int(ncoef))
    order = np.argsort(co, kind="stable")
    if ((co + need)[order][:-1] > co[order][1:]).any():
        raise ValueError("jpeg_entropy_decode: two images share coefficient storage")
    first, count = i64(images, "first_segment"), i64(images, "segments")
    if ((first < 0) | (count < 1) | (first + count > segs.size)).any():
        raise ValueError("jpeg_entropy_decode: an image's segments lie outside the table of %d" % segs.size)
    b, e, fm, m = segs["begin"], segs["end"], i64(segs, "first_mcu"), i64(segs, "mcus")
    if ((b < 0) | (b > e) | (e > int(nscan)) | (fm < 0) | (m < 1)).any():
        raise ValueError("jpeg_entropy_decode: a segment outside the scan buffer of %d bytes (or without MCUs)" % int(nscan))
    total = int(count.sum())
    starts = np.cumsum(count) - count
    idx = np.repeat(first - starts, count) + np.arange(total)             # the segments of image 0, of image 1, ...
    head = np.zeros(total, bool)
    head[starts] = True
    expect = np.where(head, 0, np.roll(fm[idx] + m[idx], 1))
    last = starts + count - 1
    if (fm[idx] != expect).any() or ((fm[idx] + m[idx])[last] != mcus).any():
        raise ValueError("jpeg_entropy_decode: the segments of an image do not cover its MCUs in sequence")
    return images, segs


def jpeg_entropy_decode_segments_host(scan, images, segs, coef):
    """ds_jpeg_entropy_decode_segments_host on NumPy arrays: decodes into coef (int16, in place) and returns the int32
    status word of every image (0 = decoded)."""
    import numpy as np
    if scan.dtype != np.uint8 or coef.dtype != np.int16 or not scan.flags.c_contiguous or not coef.flags.c_contiguous:
        raise ValueError("jpeg_entropy_decode_segments_host: scan uint8 and coef int16, both contiguous")
    images, segs = check_jpeg_scan_descs(images, segs, scan.size, coef.size)
    images, segs = np.ascontiguousarray(images), np.ascontiguousarray(segs)
    status = np.full(images.size, -1, np.int32)
    rc = _lib.load().ds_jpeg_entropy_decode_segments_host(_host_ptr(scan), scan.size, _host_ptr(images), images.size, _host_ptr(segs),
                                                          segs.size, _host_ptr(coef), coef.size, _host_ptr(status))
    if rc != 0:
        raise ValueError("ds_jpeg_entropy_decode_segments_host: bad argument (%d)" % rc)
    return status


def jpeg_entropy_decode_device(scan, images, segs, coef, images_dev=None, segs_dev=None, status=None):
    """ds_jpeg_entropy_decode_device: scan (device uint8: the entropy-coded bytes of the batch), images / segs (HOST arrays
    of ops.jpeg_scan_desc_dtype() / jpeg_segment_dtype(), checked here against the buffer sizes; images_dev / segs_dev: the
    same tables already on the device, uploaded here when None), coef (device int16, written in place: each image's own
    range only).  Returns status (device int32, one word per image, 0 = decoded; allocated when None)."""
    import numpy as np
    if not (scan.is_cuda and coef.is_cuda):
        raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
    if scan.dtype != torch.uint8 or coef.dtype != torch.int16 or not scan.is_contiguous() or not coef.is_contiguous():
        raise ValueError("jpeg_entropy_decode_device: scan must be a contiguous uint8 tensor and coef a contiguous int16 tensor")
    images, segs = check_jpeg_scan_descs(images, segs, scan.numel(), coef.numel())
    B, S = int(images.size), int(segs.size)
    if images_dev is None:
        images_dev = torch.from_numpy(np.ascontiguousarray(images).view(np.uint8)).to(coef.device)
    if segs_dev is None:
        segs_dev = torch.from_numpy(np.ascontiguousarray(segs).view(np.uint8)).to(coef.device)
    for name, t, need in (("images_dev", images_dev, B * jpeg_scan_desc_dtype().itemsize), ("segs_dev", segs_dev, S * jpeg_segment_dtype().itemsize)):
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < need:
            raise ValueError("jpeg_entropy_decode_device: %s is smaller than its table" % name)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=coef.device)
    if status.dtype != torch.int32 or not status.is_cuda or not status.is_contiguous() or status.numel() < B:
        raise ValueError("jpeg_entropy_decode_device: status must be a contiguous int32 device tensor, one word per image")
    _lib.check(_lib.load().ds_jpeg_entropy_decode_device(_p(scan), scan.numel(), _p(images_dev), B, _p(segs_dev), S, _p(coef),
                                                         coef.numel(), _p(status), _stream()), "ds_jpeg_entropy_decode_device")
    return status[:B]


# ---- the decoded-image cache: batch assembly from resident images (ds_ragged_gather) -------------------------------------------
def gather_desc_dtype():
    """NumPy view of ds_gather_desc (40 bytes): one record per image of a ds_ragged_gather launch."""
    import numpy as np
    return np.dtype([("src_offset", np.int64), ("out_offset", np.int64), ("src", np.int32), ("pitch", np.int32),
                     ("y0", np.int32), ("x0", np.int32), ("height", np.int32), ("width", np.int32)], align=True)


def check_gather_descs(desc, narena, nspill, nout):
    """Every record of the table names a source that exists (0 = arena of `narena` bytes, 1 = spill of `nspill` bytes; pass
    nspill = 0 when there is no spill buffer), its window lies inside its source row and its source buffer, its
    destination range lies inside `nout` bytes at a multiple of 4, and no two windows share output bytes: raises
    ValueError before anything is launched (the launch skips a record that does not fit and cannot see an overlap)."""
    import numpy as np
    desc = np.asarray(desc)
    if desc.dtype != gather_desc_dtype() or desc.ndim != 1 or desc.size == 0:
        raise ValueError("ragged_gather: descriptors must be a non-empty 1-D array of ops.gather_desc_dtype()")
    i64 = lambda k: desc[k].astype(np.int64)
    src, pitch, y0, x0, h, w = i64("src"), i64("pitch"), i64("y0"), i64("x0"), i64("height"), i64("width")
    so, oo = desc["src_offset"], desc["out_offset"]
    if ((src != 0) & (src != 1)).any():
        raise ValueError("ragged_gather: src must be 0 (arena) or 1 (spill)")
    n = h * w * 3
    if ((h < 1) | (w < 1) | (y0 < 0) | (x0 < 0) | (pitch < 1) | (n > 0x7fffffff)).any():
        raise ValueError("ragged_gather: a window must be at least 1 x 1 pixels, at a non-negative origin, below 2**31 bytes")
    nsrc = np.where(src == 1, int(nspill), int(narena))
    last = (y0 + h - 1) * pitch + (x0 + w) * 3
    if (((x0 + w) * 3 > pitch) | (so < 0) | (so > nsrc) | (last > nsrc - so)).any():
        i = int(np.flatnonzero(((x0 + w) * 3 > pitch) | (so < 0) | (so > nsrc) | (last > nsrc - so))[0])
        raise ValueError("ragged_gather: the window of record %d leaves its source (%s of %d bytes)"
                         % (i, "spill" if src[i] else "arena", int(nsrc[i])))
    if ((oo < 0) | (oo + n > int(nout))).any():
        raise ValueError("ragged_gather: a window outside the output buffer of %d bytes" % int(nout))
    if (oo % 4 != 0).any():
        raise ValueError("ragged_gather: out_offset must be a multiple of 4")
    order = np.argsort(oo, kind="stable")
    if ((oo + n)[order][:-1] > oo[order][1:]).any():
        raise ValueError("ragged_gather: two windows overlap in the output buffer")
    return desc


def ragged_gather_host(arena, spill, desc, out):
    """ds_ragged_gather_host on NumPy arrays: arena / spill (uint8; spill may be None) -> the windows of `desc` in out
    (uint8, in place).  Returns out."""
    import numpy as np
    for a in (arena, spill, out):
        if a is not None and (a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous):
            raise ValueError("ragged_gather_host: arena, spill and out must be contiguous 1-D uint8 arrays")
    desc = np.ascontiguousarray(check_gather_descs(desc, arena.size, 0 if spill is None else spill.size, out.size))
    rc = _lib.load().ds_ragged_gather_host(_host_ptr(arena), arena.size, None if spill is None else _host_ptr(spill),
                                           0 if spill is None else spill.size, _host_ptr(desc), desc.size, _host_ptr(out), out.size)
    if rc != 0:
        raise ValueError("ds_ragged_gather_host: bad argument (%d)" % rc)
    return out


def ragged_gather(arena, spill, desc, out, desc_dev=None):
    """ds_ragged_gather: arena / spill (device uint8; spill may be None when no record names it), desc (HOST array of
    ops.gather_desc_dtype(), checked here), out (device uint8, written in place: only the windows' bytes), desc_dev (the
    table already on the device; uploaded here when None).  Returns out."""
    import numpy as np
    for t in (arena, spill, out):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("ragged_gather: arena, spill and out must be contiguous uint8 tensors")
    desc = check_gather_descs(desc, arena.numel(), 0 if spill is None else spill.numel(), out.numel())
    B = int(desc.size)
    if desc_dev is None:
        desc_dev = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).to(out.device)
    if not desc_dev.is_cuda or not desc_dev.is_contiguous() or desc_dev.numel() * desc_dev.element_size() < B * gather_desc_dtype().itemsize:
        raise ValueError("ragged_gather: desc_dev is smaller than the descriptor table")
    _lib.check(_lib.load().ds_ragged_gather(_p(arena), arena.numel(), _p(spill), 0 if spill is None else spill.numel(),
                                            _p(desc_dev), B, _p(out), out.numel(), _stream()), "ds_ragged_gather")
    return out


# ---- the Mixed_5b feature cache: batch assembly from resident tables (ds_rows_gather) ------------------------------------------
class RowsGather:
    """One ds_rows_gather launch shape: the ds_rows_table array (host side; it travels by value in the launch) of up to 8
    (src, dst) pairs whose rows are gathered by one index vector.  src [nrows, ...] and dst [n, ...] are contiguous device
    tensors of one dtype with equal row shapes; the addresses are read at construction, so build it anew when a buffer is
    re-allocated."""

    def __init__(self, pairs):
        pairs = list(pairs)
        if not 1 <= len(pairs) <= 8:
            raise ValueError("rows_gather: 1 to 8 tables")
        nrows, n = pairs[0][0].shape[0], pairs[0][1].shape[0]
        self.tables = (_lib.RowsTable * len(pairs))()
        for t, (src, dst) in zip(self.tables, pairs):
            for x in (src, dst):
                if not x.is_cuda:
                    raise RuntimeError("tumblr_emotions_amd kernels need CUDA/HIP tensors; there is no CPU fallback")
            if src.dtype != dst.dtype or src.shape[1:] != dst.shape[1:] or not src.is_contiguous() or not dst.is_contiguous() \
                    or src.dim() < 1 or src.shape[0] != nrows or dst.shape[0] != n:
                raise ValueError("rows_gather: a table and its destination are contiguous, of one dtype and row shape, and "
                                 "all tables share their row counts")
            row_bytes = src[0].numel() * src.element_size() if nrows else 0
            if row_bytes < 4 or row_bytes % 4:
                raise ValueError("rows_gather: row_bytes must be a positive multiple of 4, not %d" % row_bytes)
            t.src, t.dst, t.row_bytes = src.data_ptr(), dst.data_ptr(), row_bytes
        self.nrows, self.n, self.keep = int(nrows), int(n), pairs

    def run(self, index):
        """dst_t[i] = src_t[index[i]] for every table: index is a contiguous int64 device vector of n entries inside
        [0, nrows) (validated by whoever generated it: a row whose index is outside is left without a store)."""
        if not index.is_cuda or index.dtype != torch.int64 or index.dim() != 1 or index.shape[0] != self.n or not index.is_contiguous():
            raise ValueError("rows_gather: index must be a contiguous int64 device vector of %d entries" % self.n)
        _lib.check(_lib.load().ds_rows_gather(self.tables, len(self.tables), _p(index), self.n, self.nrows, _stream()),
                   "ds_rows_gather")


def rows_gather(pairs, index):
    """ds_rows_gather once: pairs = [(src, dst), ...] (see RowsGather), index int64 [n] on the device."""
    RowsGather(pairs).run(index)


def rows_gather_host(pairs, index, nrows=None):
    """ds_rows_gather_host on NumPy arrays: pairs = [(src, dst), ...] with dst written in place, index int64 [n].  The arrays
    need no alignment (views at odd byte offsets are fine) but must be C-contiguous; nrows defaults to the tables' rows."""
    import numpy as np
    pairs = list(pairs)
    if not 1 <= len(pairs) <= 8:
        raise ValueError("rows_gather_host: 1 to 8 tables")
    index = np.asarray(index)
    if index.dtype != np.int64 or index.ndim != 1 or not index.flags.c_contiguous:
        raise ValueError("rows_gather_host: index must be a contiguous int64 vector")
    tables = (_lib.RowsTable * len(pairs))()
    for t, (src, dst) in zip(tables, pairs):
        if not src.flags.c_contiguous or not dst.flags.c_contiguous or src.dtype != dst.dtype or src.shape[1:] != dst.shape[1:] \
                or dst.shape[0] != index.shape[0] or src.shape[0] != pairs[0][0].shape[0]:
            raise ValueError("rows_gather_host: a table and its destination are contiguous, of one dtype and row shape")
        t.src, t.dst, t.row_bytes = src.ctypes.data, dst.ctypes.data, src[0].nbytes
    rc = _lib.load().ds_rows_gather_host(tables, len(pairs), index.ctypes.data, index.shape[0],
                                         pairs[0][0].shape[0] if nrows is None else nrows)
    if rc != 0:
        raise ValueError("ds_rows_gather_host: %s (%d)" % (_lib.load().ds_last_error().decode(), rc))
