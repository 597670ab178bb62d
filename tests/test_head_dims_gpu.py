"""JointHeadEngine and TextHeadEngine on a store of their own, across the thresholds at which ops.head_gemm_plan and the engines
switch launch forms: M <= 512 / K >= 256 / K >= 512 (plain plan, 4 or 8 split-K slabs), split-K slices that are ragged or own no
K-tile at all, the grouped chain and the cross entropy in the W_softmax combine (B <= 512, nc <= 32; its second trip over rows
256 ..), ds_colsum's one-launch and two-stage forms.  Every result is held against head_ref (NumPy fp64 on the same fp32 inputs)
at the kernel tests' gate for these GEMMs, 2e-4 * max|ref| per tensor (test_head_group_gpu.REL,
test_split_gemm_with_slab_epilogue_matches_the_single_launch), dlogits also per row against the row's own maximum; grouped and
ungrouped runs must agree bit for bit.  Every case asserts the form it reached; the closing test asserts that together they
reached all of them (head_ref.ALL_FORMS).

Every buffer the engines write is filled with NaN between the plan-building forward and the measured one (outputs, gradients,
split-K slabs, workspaces), and the padding columns of the strided feature tensors hold 1e3: a slab nobody writes, a column
nobody combines or a read past a row shows up at every K, not only where torch.empty happens to hold zeros.

The fp64 reference follows the ReLU decisions of the HIP forward pass (as test_model_gpu._check_step does for the image tower):
a unit whose pre-activation is within rounding of zero may legitimately differ; the test asserts that it differs nowhere else.

Per-row gate of dlogits: REL * max|ref row| + head_ref.ce_row_floor(nc, 1 / B) = (nc + 7) u / B, the absolute rounding of
(softmax - onehot) / B derived there: where the label takes nearly all the probability the whole row is smaller than the
rounding of softmax itself, whatever the kernel (u = 2^-24).

On an MI355X the worst error / bound ratio (every case prints its own) is 0.074, a row of dlogits at nc = 2, B = 257; the
per-tensor gates stay below 0.008, the single slabs below 0.002; no ReLU decision differed; the file takes 4.0 s."""
import numpy as np
import pytest
import torch

import head_ref as HR

pytestmark = pytest.mark.gpu

NAN = float("nan")
REACHED = set()
WORST = HR.Worst()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _strided(rng, B, n, pad):
    full = np.full((B, n + pad), 1e3, np.float32)
    full[:, :n] = rng.normal(size=(B, n))
    return torch.from_numpy(full).cuda()[:, :n]


def _splits_of(ops, plan):
    return plan.splits if isinstance(plan, ops.SplitGemm) else 0


def _poison(ops, head, store, names):
    for t in names:
        getattr(head, t).fill_(NAN)
    store.grad.fill_(NAN)
    head.ws.fill_(NAN)
    head.colsum_scratch.fill_(NAN)
    for p in vars(head).values():
        if isinstance(p, ops.SplitGemm):
            p.slabs.fill_(NAN)


def _run_joint(case, group):
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.engine_text import JointHeadEngine
    from tumblr_emotions_amd.params import ParamStore
    B, im, tx, fc, nc = case
    rng = np.random.RandomState(1000 + B + 3 * im + 5 * tx + 7 * fc + 11 * nc)
    w = dict(W_fc=rng.normal(size=(im + tx, fc)) * 0.05, b_fc=rng.normal(size=fc) * 0.1,
             W_softmax=rng.normal(size=(fc, nc)) * 0.1, b_softmax=rng.normal(size=nc) * 0.1)
    store = ParamStore()
    head = JointHeadEngine(store, im, tx, fc, nc)
    store.finalize()
    for k, v in w.items():
        store.view(k).copy_(torch.from_numpy(v.astype(np.float32)))
    head.group = group
    f_im, f_tx = _strided(rng, B, im, 8), _strided(rng, B, tx, 4)
    assert (f_im.stride(0), f_tx.stride(0)) == (im + 8, tx + 4)
    labels = torch.from_numpy(rng.randint(0, nc, size=B)).cuda()
    loss, dlogits = torch.full((1,), NAN, device="cuda"), torch.full((B, nc), NAN, device="cuda")
    head.forward(f_im, f_tx)                      # builds the plans of this batch size (SentimentNet._step_body asks them next)
    plans = {k: _splits_of(ops, getattr(head, k)) for k in ("fc_im", "fc_tx", "sm", "sm_dgrad", "im_dgrad", "tx_dgrad")}
    grouped, fused = head.grouped(), head.ce_fused()
    _poison(ops, head, store, ("dense", "ddense", "logits", "d_im", "d_tx"))
    if fused:
        logits = head.forward(f_im, f_tx, ce=(labels, loss, dlogits))
    else:
        logits = head.forward(f_im, f_tx)
        ops.softmax_ce(logits, labels, B, nc, 1.0, None, loss, dlogits)
    d_im, d_tx = head.backward(dlogits)
    torch.cuda.synchronize()
    out = dict(dense=_np(head.dense), logits=_np(logits), loss=_np(loss), dlogits=_np(dlogits), d_im=_np(d_im), d_tx=_np(d_tx))
    for k in w:
        out[k] = _np(store.grad_view(k))
    # (the grouped chain runs ONE GEMM through W_fc, fc_dgrad, in place of im_dgrad and tx_dgrad: their slabs stay unused)
    unused = ("im_dgrad", "tx_dgrad") if grouped else ()
    slabs = {k: _np(getattr(head, k).slabs) for k, s in plans.items() if s and k not in unused}
    if grouped:
        slabs["fc_dgrad"] = _np(head.fc_dgrad.slabs)
    w32 = {k: _np(store.view(k)).astype(np.float64) for k in w}
    return out, plans, grouped, fused, slabs, (_np(f_im).astype(np.float64), _np(f_tx).astype(np.float64), w32, _np(labels))


def _check_against_ref(out, ref, B, what):
    """Returns the case's own worst error / bound ratio (and keeps the module's)."""
    worst = HR.Worst()
    for k in ("dense", "logits", "dlogits", "W_fc", "b_fc", "W_softmax", "b_softmax", "d_im", "d_tx"):
        if k in ref:
            HR.check_close(out[k], ref[k], "%s %s" % (what, k), worst=worst)
    HR.check_close(out["loss"], [ref["loss"]], what + " loss", worst=worst)
    HR.check_rows(out["dlogits"], ref["dlogits"], what + " dlogits per row", HR.REL,
                  floor=HR.ce_row_floor(ref["dlogits"].shape[1], 1.0 / B), worst=worst)
    WORST.take(worst.ratio, worst.what)
    return worst


@pytest.mark.parametrize("case", HR.JOINT_CASES, ids=lambda c: "B%d-im%d-tx%d-fc%d-nc%d" % c)
def test_joint_head_across_the_plan_thresholds(case):
    B, im, tx, fc, nc = case
    want_plans, want_grouped, want_fused, forms = HR.joint_forms(*case)
    what = "joint B=%d im=%d tx=%d fc=%d nc=%d" % case
    out, plans, grouped, fused, slabs, (f_im, f_tx, w, labels) = _run_joint(case, True)
    assert plans == want_plans, (plans, want_plans)
    assert (grouped, fused) == (want_grouped, want_fused), (grouped, fused)
    ref = HR.joint_head(f_im, f_tx, w["W_fc"], w["b_fc"], w["W_softmax"], w["b_softmax"], labels, decisions=out["dense"] > 0)
    flipped = (out["dense"] > 0) != (ref["pre"] > 0)
    assert float(np.abs(ref["pre"][flipped]).max(initial=0.0)) <= HR.REL * np.abs(ref["pre"]).max(), "a ReLU decision far from 0"
    worst = _check_against_ref(out, ref, B, what)
    # a split that owns no K-tile leaves a slab of exact zeros (not the NaN it held before)
    ks = dict(fc_im=im, fc_tx=tx, sm=fc, sm_dgrad=nc, im_dgrad=fc, tx_dgrad=fc, fc_dgrad=fc)
    for k, s in slabs.items():
        assert not np.isnan(s).any(), k
        if HR.split_tiles(ks[k], s.shape[0])[-1] == 0:
            assert not s[-1].any(), "%s: the empty last slice's slab is not zero" % k
    if grouped:
        off, plans2, grouped2, fused2, _, _ = _run_joint(case, False)
        assert plans2 == plans and not grouped2 and not fused2
        for k in out:
            HR.check_bits(out[k], off[k], "%s: %s with head.group on / off" % (what, k))
        forms = forms | {"ungrouped", "ce-separate"}
    REACHED.update(forms)
    print("%s: plans %s grouped %s fused %s; %s" % (what, plans, grouped, fused, worst))


@pytest.mark.parametrize("case", HR.TEXT_CASES, ids=lambda c: "B%d-H%d-nc%d" % c)
def test_text_head_across_the_plan_thresholds(case):
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.engine_text import TextHeadEngine
    from tumblr_emotions_amd.params import ParamStore
    B, H, nc = case
    want_plans, forms = HR.text_forms(*case)
    what = "text B=%d H=%d nc=%d" % case
    rng = np.random.RandomState(2000 + B + 3 * H + 5 * nc)
    store = ParamStore()
    head = TextHeadEngine(store, H, nc)
    store.finalize()
    store.view("W_softmax").copy_(torch.from_numpy((rng.normal(size=(H, nc)) * 0.1).astype(np.float32)))
    store.view("b_softmax").copy_(torch.from_numpy((rng.normal(size=nc) * 0.1).astype(np.float32)))
    h = torch.from_numpy(rng.normal(size=(B, H)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.randint(0, nc, size=B)).cuda()
    loss, dlogits = torch.full((1,), NAN, device="cuda"), torch.full((B, nc), NAN, device="cuda")
    head.forward(h)
    plans = {k: _splits_of(ops, getattr(head, k)) for k in ("sm", "sm_dgrad")}
    assert plans == want_plans, (plans, want_plans)
    _poison(ops, head, store, ("logits", "d_tx"))
    logits = head.forward(h)
    ops.softmax_ce(logits, labels, B, nc, 1.0, None, loss, dlogits)
    d_tx = head.backward(dlogits)
    torch.cuda.synchronize()
    out = dict(logits=_np(logits), loss=_np(loss), dlogits=_np(dlogits), d_tx=_np(d_tx),
               W_softmax=_np(store.grad_view("W_softmax")), b_softmax=_np(store.grad_view("b_softmax")))
    ref = HR.text_head(_np(h).astype(np.float64), _np(store.view("W_softmax")).astype(np.float64),
                       _np(store.view("b_softmax")).astype(np.float64), _np(labels))
    worst = _check_against_ref(out, ref, B, what)
    if plans["sm"] and HR.split_tiles(H, plans["sm"])[-1] == 0:
        assert not _np(head.sm.slabs)[-1].any()
    REACHED.update(forms)
    print("%s: plans %s; %s" % (what, plans, worst))


@pytest.mark.parametrize("K", [260, 300, 520, 560, 648, 776])
def test_split_k_slices_ragged_and_empty(K):
    """head_gemm_plan alone, M in {1, 512} x N in {15, 512} x both weight orientations, slabs NaN before the run: the combined
    result against fp64 at 2e-4, every slab against the partial product of the K range its split owns (the same gate, against
    the full product's magnitude), and the slab of a split without a K-tile exactly zero."""
    from tumblr_emotions_amd import ops
    splits = HR.plan_splits(1, K)
    tiles, ranges = HR.split_tiles(K, splits), HR.split_ranges(K, splits)
    assert splits == (8 if K >= 512 else 4) and (tiles[-1] == 0) == (K >= 512)
    worst = HR.Worst()
    for M in (1, 512):
        for N in (15, 512):
            for transposed in (False, True):
                rng = np.random.RandomState(K + M + N + transposed)
                a = rng.normal(size=(M, K)).astype(np.float32)
                w = (rng.normal(size=(N, K) if transposed else (K, N)) * 0.05).astype(np.float32)
                ad = torch.from_numpy(np.pad(a, ((0, 0), (0, 8)), constant_values=1e3)).cuda()
                wd = torch.from_numpy(w).cuda()
                plan = ops.head_gemm_plan(M, K, N, K + 8, N + 4, K if transposed else N, transposed_w=transposed, device="cuda")
                assert isinstance(plan, ops.SplitGemm) and plan.splits == splits
                plan.slabs.fill_(NAN)
                out = torch.full((M, N + 4), 5.0, device="cuda")
                plan.run(ops._p(ad), ops._p(wd), ops._p(out))
                torch.cuda.synchronize()
                a64, w64 = a.astype(np.float64), (w.T if transposed else w).astype(np.float64)
                full = a64 @ w64
                what = "K=%d M=%d N=%d %s" % (K, M, N, "W^T" if transposed else "W")
                HR.check_close(_np(out)[:, :N], full, what, worst=worst)
                assert bool((out[:, N:] == 5.0).all()), what + ": row padding written"
                slabs = _np(plan.slabs)
                scale = float(np.abs(full).max())
                for s, (k0, k1) in enumerate(ranges):
                    if k1 == k0:
                        assert not slabs[s].any(), "%s: slab %d of a split without K-tiles is not zero" % (what, s)
                    else:
                        HR.check_bound(slabs[s], a64[:, k0:k1] @ w64[k0:k1], HR.REL * scale, "%s slab %d" % (what, s), worst)
    REACHED.update({"slice-" + HR.slice_form(K, splits), "split%d" % splits})
    print("K=%d tiles %s: %s" % (K, tiles, worst))
    WORST.take(worst.ratio, worst.what)


def test_the_cases_reach_every_launch_form():
    """Run after the cases above (same module): together they reached every form named in head_ref.ALL_FORMS -- a case that
    silently lands on another plan fails its own assertion, a form nobody reaches fails here."""
    if not REACHED:
        pytest.skip("needs the cases of this module in the same session")      # (only when selected alone)
    assert REACHED == HR.ALL_FORMS, sorted(HR.ALL_FORMS - REACHED)
    print("test_head_dims_gpu: %s" % WORST)
