"""Free-running multi-step training on the GPU against the fp64 oracle.

The one-step tests (tests/test_model_gpu.py) start every step from a freshly loaded state: their second step first
copies the oracle's state INTO the net, which goes through load_state_dict() -> after_load() and so rebuilds every
prepared filter form, drops a captured graph and rewrites variables, Adam slots and `step` from outside.  Here the copy
goes the other way.  Before every step the HIP state (variables, frozen variables, moving statistics, Adam m / v) is
copied into the oracle -- fp32 -> fp64 is exact -- and the net is never touched between steps.  Both sides then start
every step from bit-identical state, so the smooth one-step gates of test_model_gpu._check_step apply unchanged (the
TF-Adam drift that forced the other direction cannot build up), while the net runs a genuine trajectory and carries
everything it derives from its state itself: the prepared filter forms of the trainable layers (G g G^T, bf16 orders),
each layer's BatchNorm statistics pivot (its previous batch mean), `step` / lr_t / the dropout seed and their device
copies under a captured graph, the moving statistics and Adam slots as it accumulated them, the text tower's sort and
workspace state.  Every step has another batch and another learning rate, so a stale scalar or pointer cannot hide.

On top of _check_step's gates the well-resolved entries of every trainable variable (|g| > 1e-2 max|g|) are held to
the first step's rule at EVERY step (>= 99 % within 1e-5): both sides share the same non-zero Adam slots here.

The planted-fault tests at the end break the carried state from Python (monkeypatch only; every launch stays a valid
launch on valid buffers) and assert that the same check raises at the step where the fault first shows.

Measured on an MI355X (each test prints these per step; gates in brackets), per step 1 / 2 / 3 / 4:

  configuration     max|dlogits| [1e-3]          worst gradient rel. L2 [tol]          worst resolved entry [1e-5]
  text small        4.4e-8 5.6e-8 4.8e-8 4.4e-8  2.4e-7 1.5e-7 1.3e-7 1.7e-7 [1e-3]    2.2e-8 1.7e-8 1.6e-8 1.5e-8
  text defaults     1.0e-7 9.7e-8 9.1e-8 5.5e-8  1.8e-7 1.6e-7 1.8e-7 1.7e-7 [1e-3]    2.1e-8 1.7e-8 1.5e-8 1.5e-8
  joint, dropout    2.4e-5 3.3e-5 2.7e-5 2.7e-5  1.5e-4 1.1e-4 1.2e-4 1.7e-4 [2e-3]    2.1e-8 9.3e-7 3.4e-7 8.9e-8
  image train_all   3.4e-5 3.4e-5 4.3e-5         8.1e-5 7.4e-5 7.6e-5        [1e-3]    2.1e-8 7.9e-7 1.9e-7
  captured joint    2.8e-5 2.1e-5 1.8e-5 2.8e-5  1.4e-4 1.5e-4 1.3e-4 1.1e-4 [2e-3]    2.1e-8 8.9e-7 2.4e-7 1.2e-7
  captured text     4.6e-8 3.4e-8 3.4e-8 3.7e-8  2.0e-7 1.5e-7 1.5e-7 1.5e-7 [1e-3]    2.1e-8 1.7e-8 1.5e-8 1.5e-8
  joint, detours    1.8e-5 3.3e-5 1.6e-5         1.7e-4 1.0e-4 1.3e-4        [2e-3]    2.1e-8 7.9e-7 3.2e-7

100 % of the resolved entries were within 1e-5 at every step of every configuration (no bound had to be re-derived),
|dloss| <= 1.1e-5 [1e-3], moving statistics <= 7e-8 [1e-5], the two eval-mode predicts 8.6e-8 / 6.4e-8 [1e-3].  bf16
(logits [5e-2] / loss [1e-2] / median gradient [0.2]): 3.0e-2 / 5.3e-4 / 0.16, 2.9e-2 / 1.1e-3 / 0.10, 4.0e-2 / 8.4e-3 /
0.15 -- the third step's loss sits close to its gate.

Out of scope: dtype='fp8' (its oracle would need the per-step amax records) and data parallelism (it has its own clone
oracle, tests/test_dp_gpu.py).
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import tf_semantics as S
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

STEM = "InceptionV1/Conv2d_1a_7x7/weights"
EMB = "Text/W_embedding"


# ---- inputs (no GPU needed: the oracle-only margins in the planted tests' docstrings were taken with these) --------------

def step_lr(lr0, k):
    """learning rate of step k = 1, 2, ...: halves every step"""
    return lr0 * 0.5 ** (k - 1)


def step_batch(k, B, T, V, seed, with_images):
    """batch of step k: new samples every step; with text, the shortest (1) and the full (T) length sit in other rows
    every step and the other lengths change too"""
    b = S.synthetic_batch(B, T, V, seed=seed + 17 * k, with_images=with_images)
    if B >= 2:
        b["seq_lens"][k % B], b["seq_lens"][(k + 1) % B] = 1, T
        rows = np.arange(T)[None, :] >= b["seq_lens"][:, None]
        fresh = np.random.RandomState(seed + 17 * k + 1).randint(0, V, size=b["texts"].shape)
        b["texts"] = np.where(rows, V, np.where(b["texts"] == V, fresh, b["texts"])).astype(np.int64)
    return b


def text_setup(V, D, H, T, seed):
    rng = np.random.RandomState(seed)
    params = R.make_params("text", rng, num_classes=15, embed_dim=D, rnn_size=H, dtype=np.float64)
    params["Text/rnn/basic_lstm_cell/bias"] = rng.normal(0, 0.1, size=4 * H)
    return params, S.synthetic_embedding(V, D).astype(np.float64)


JOINT = dict(V=60, D=20, H=32, T=12)


def joint_setup(seed):
    rng = np.random.RandomState(seed)
    params = R.make_params("joint", rng, num_classes=15, im_features_size=256, embed_dim=JOINT["D"], rnn_size=JOINT["H"],
                           fc_size=512, dtype=np.float64)
    for k in params:
        if k.endswith("beta"):
            params[k] = rng.normal(0, 0.1, size=params[k].shape)
    return params, S.synthetic_embedding(JOINT["V"], JOINT["D"]).astype(np.float64)


# ---- HIP state -> oracle --------------------------------------------------------------------------------------------------

def _slots(net, which):
    """Adam slot `which` of every trainable variable under its TF name (fused tensors split, the stem as [7,7,3,64])"""
    out = {}
    for e in net.store.entries.values():
        if not e.trainable:
            continue
        t = net.store.slot_view(e.name, which).detach().cpu()
        if e.columns:
            for (n, c0, c1) in e.columns:
                out[n] = t[..., c0:c1].contiguous().numpy()
        else:
            out[e.name] = t.numpy().copy()
    if STEM in out:
        out[STEM] = out[STEM][:, :, :3, :].copy()
    return out


def sync_oracle_from_net(net, ref, step):
    """The oracle takes over the net's whole optimiser state, exactly (fp32 -> fp64); the net is only read."""
    torch.cuda.synchronize()
    sd = net.state_dict()
    m, v = _slots(net, "m"), _slots(net, "v")
    assert set(ref.adam_m) <= set(m) and set(ref.p) <= set(sd)
    with torch.no_grad():
        for name, t in ref.p.items():      # in place: requires_grad and (trainable embedding) ref.embedding's identity stay
            t.copy_(torch.from_numpy(np.ascontiguousarray(sd[name])).reshape(t.shape))
        if ref.embedding is not None and EMB not in ref.p:
            ref.embedding.copy_(torch.from_numpy(sd[EMB]).reshape(ref.embedding.shape))
        for name in ref.trainable:
            ref.adam_m[name].copy_(torch.from_numpy(m[name]).reshape(ref.adam_m[name].shape))
            ref.adam_v[name].copy_(torch.from_numpy(v[name]).reshape(ref.adam_v[name].shape))
    if step > 0:      # the run really carries optimiser state: every trainable variable has been moved by Adam
        assert all(np.abs(v[n]).max() > 0 for n in ref.trainable if n != EMB), "empty Adam slots after %d steps" % step
    ref.step = step


def _refill(dev, batch):
    for k, t in dev.items():
        t.copy_(torch.from_numpy(np.ascontiguousarray(batch[k])))


def free_run(net, ref, batches, lr0, label, dev=None, hip_mask=False, grad_tol=1e-3, after_step=None):
    """Steps 1..K of the check.  `dev`: static device tensors refilled in place (captured step).  after_step(k): a hook
    for the interleaved calls and the planted faults.  A failed gate is re-raised with the step number in front."""
    from test_model_gpu import _check_step
    masks = []
    for k, batch in enumerate(batches, 1):
        lr = step_lr(lr0, k)
        try:
            # the test keeps the count: a net that loses a step must not take the oracle with it
            assert net.step == k - 1, "net.step is %d before step %d" % (net.step, k)
            sync_oracle_from_net(net, ref, k - 1)
            if dev is not None:
                _refill(dev, batch)
            rep = {}
            _check_step(net, ref, batch, lr, first=(k == 1), grad_tol=grad_tol, dev_batch=dev, hip_mask=hip_mask,
                        resolved_every_step=True, report=rep)
        except AssertionError as e:
            raise AssertionError("step %d: %s" % (k, e)) from e
        print("%s step %d (lr %.2e): max|dlogits| %.3e (gate 1e-3), |dloss| %.3e (1e-3), worst gradient relative L2 %.3e "
              "(%.0e; %s), variables max %.3e (%.3e), well-resolved entries within 1e-5: %.4f, worst %.3e (%s), moving "
              "statistics %.3e (1e-5)" % (label, k, lr, rep["logits"], rep["loss"], rep["grad"][0], grad_tol, rep["grad"][1],
                                          rep["var"][0], 2.5 * lr + 1e-6, rep["resolved"][0], rep["resolved_max"][0],
                                          rep["resolved_max"][1], rep["moving"]))
        if hip_mask:
            masks.append(net.image.mask.detach().clone())
        if after_step is not None:
            after_step(k)
    assert net.step == len(batches)
    if hip_mask:      # a fresh Bernoulli(0.8) mask every step (the bound of test_kernels_gpu.test_avgpool_dropout)
        for a, b in itertools.combinations(masks, 2):
            assert not torch.equal(a, b), "two steps drew the same dropout mask"
        for m in masks:
            assert set(m.unique().tolist()) <= {0.0, 1.0} and abs(float(m.mean()) - 0.8) < 0.03


def _text_nets(V, D, H, T, seed):
    from tumblr_emotions_amd.net import SentimentNet
    params, emb = text_setup(V, D, H, T, seed)
    ref = R.DeepSentimentRef(params, emb, "text", torch.float64)
    net = SentimentNet(mode="text", nb_emotions=15, rnn_size=H, vocab_size=V, embedding_dim=D, post_size=T)
    net.load_state_dict(dict(params, **{EMB: emb}))
    return net, ref


def _joint_nets(seed, **kw):
    from tumblr_emotions_amd.net import SentimentNet
    params, emb = joint_setup(seed)
    ref = R.DeepSentimentRef(params, emb, "joint", torch.float64)
    net = SentimentNet(mode="joint", nb_emotions=15, im_features_size=256, rnn_size=JOINT["H"], fc_size=512,
                       vocab_size=JOINT["V"], embedding_dim=JOINT["D"], post_size=JOINT["T"], **kw)
    net.load_state_dict(dict(params, **{EMB: emb}))
    return net, ref


def _joint_batches(K, B, seed):
    return [step_batch(k, B, JOINT["T"], JOINT["V"], seed, True) for k in range(1, K + 1)]


def _device(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


# ---- 1: text ---------------------------------------------------------------------------------------------------------------

TEXT_DIMS = {"small": (40, 12, 16, 9, 8), "reference-defaults": (100, 50, 64, 50, 5)}


@pytest.mark.parametrize("dims", list(TEXT_DIMS))
def test_text_free_run_matches_oracle_every_step(dims):
    """Four free-running text steps: the LSTM's workspace counters and length sort with other lengths every step (1 and T
    included), lr_t with t > 1 as the net computes it, the text variables' Adam slots as the net accumulated them."""
    V, D, H, T, B = TEXT_DIMS[dims]
    net, ref = _text_nets(V, D, H, T, seed=81)
    batches = [step_batch(k, B, T, V, 200, False) for k in range(1, 5)]
    assert len({tuple(b["seq_lens"]) for b in batches}) == 4
    free_run(net, ref, batches, 1e-3, "text/" + dims)


# ---- 2: joint, dropout on with the net's own masks -----------------------------------------------------------------------

def test_joint_free_run_with_generated_dropout_matches_oracle_every_step():
    """Four free-running joint steps at B = 4 with dropout on: the oracle gets the mask the net drew (net.image.mask).
    Pins down Mixed_5c's prepared filters redone every step, every layer's statistics pivot from the second step on and the
    per-step dropout seed.  Gradient tolerance 2e-3: the B = 4 figure test_joint_step_matches_oracle documents."""
    net, ref = _joint_nets(71)
    assert net.image.keep == pytest.approx(0.8)
    free_run(net, ref, _joint_batches(4, 4, 100), 1e-3, "joint", hip_mask=True, grad_tol=2e-3)


# ---- 3: every conv trainable ------------------------------------------------------------------------------------------------

def test_full_fine_tuning_free_run_matches_oracle_every_step():
    """train_all=True, B = 3, three steps: all 57 layers' prepared forms (the stem and the fused 1x1 groups included) must
    follow Adam every step -- the once-per-load cache of a frozen layer must not be used for any of them."""
    from tumblr_emotions_amd.net import SentimentNet
    rng = np.random.RandomState(72)
    B = 3
    params = R.make_params("image", rng, num_classes=15, dtype=np.float64)
    for k in params:
        if k.endswith("beta"):
            params[k] = rng.normal(0, 0.1, size=params[k].shape)
    ref = R.DeepSentimentRef(params, None, "image", torch.float64, train_all=True)
    net = SentimentNet(mode="image", nb_emotions=15, train_all=True)
    net.load_state_dict(params)
    assert all(l.trainable for l in net.image.layers) and STEM in ref.trainable
    batches = [S.synthetic_batch(B, 8, 10, seed=300 + k) for k in range(3)]
    free_run(net, ref, batches, 1e-3, "image/train_all", hip_mask=True)


# ---- 4: the captured step ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["joint", "text"])
def test_captured_free_run_matches_oracle_every_step(mode):
    """capture_step before the first step, then four replays against the oracle with the same gates: Adam's lr_t and the
    dropout seed come from device memory (lr_t_dev, seed_dev), the weight transforms run inside the capture, and the batch
    is refilled in place so that the graph key holds.  The graph must still be there after the last step."""
    from hip_decisions import keep_activations
    if mode == "joint":
        net, ref = _joint_nets(73)
        batches = _joint_batches(4, 4, 400)
    else:
        V, D, H, T, B = TEXT_DIMS["small"]
        net, ref = _text_nets(V, D, H, T, seed=83)
        batches = [step_batch(k, B, T, V, 500, False) for k in range(1, 5)]
    keep_activations(net)      # (before the capture: it re-allocates, which would drop the graph)
    dev = _device(batches[0])
    assert net.capture_step(dev) and net.step == 0
    free_run(net, ref, batches, 1e-3, "captured/" + mode, dev=dev, hip_mask=(mode == "joint"),
             grad_tol=2e-3 if mode == "joint" else 1e-3)
    assert net._graph is not None, "the captured step was dropped on the way"


# ---- 5: detours between the steps -----------------------------------------------------------------------------------------

def _check_eval_predict(net, batch, what):
    """predict(is_training=False) against the oracle in eval mode built from the HIP state of this moment (tolerance of
    test_frontends_gpu.test_inference_mode_matches_oracle_moving_statistics); evaluation changes no variable."""
    before = net.state_dict()
    sd = dict(before)
    emb = sd.pop(EMB)
    ref = R.DeepSentimentRef(sd, emb, "joint", torch.float64, is_training=False)
    with torch.no_grad():
        want = ref.forward(batch).numpy()
    got = net.predict(_device(batch), is_training=False).cpu().numpy()
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want).max()
    print("%s: eval-mode max|dlogits| %.3e (gate %.3e)" % (what, err, 1e-3 * scale))
    assert err <= 1e-3 * scale, what
    after = net.state_dict()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k])
    assert net.image.training and net.image.update_moving


def test_joint_free_run_survives_predict_and_input_gradient_between_steps():
    """step, predict(is_training=False) on another batch, step, input_gradient, step, predict(is_training=False): every
    predict must match the eval-mode oracle on the moving statistics as training has moved them, and the steps keep
    passing -- pivots, prepared filters and buffers survive the detours (input_gradient re-allocates the tower twice)."""
    net, ref = _joint_nets(74)
    B = 4
    other = _joint_batches(3, B, 650)

    def detour(k):
        if k in (1, 3):
            _check_eval_predict(net, other[k - 1], "after step %d" % k)
        else:
            logits, dimg = net.input_gradient(_device(other[1]), 3)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(dimg).all()) and float(dimg.abs().max()) > 0

    free_run(net, ref, _joint_batches(3, B, 600), 1e-3, "joint/detours", hip_mask=True, grad_tol=2e-3, after_step=detour)


# ---- 6: bf16 multiplies, centred bf16 z storage ---------------------------------------------------------------------------

def _pivots(net):
    return {sc: l.mean[c0:c1].detach().cpu().double() for l in net.image.layers for (sc, c0, c1) in l.scopes}


def test_joint_bf16_free_run_matches_bf16_emulating_oracle_every_step():
    """dtype='bf16', B = 8, three free-running steps against the bf16-emulating oracle with the tolerances of
    test_joint_step_bf16_multiply_matches_bf16_emulating_oracle (logits 5e-2, loss 1e-2, median gradient relative L2 0.2).
    From the second step on the stored bf16(z - pivot) is centred about each layer's previous batch mean, not the moving
    mean: the pivots are read from the net before the step and handed to the oracle (DeepSentimentRef.z_pivots)."""
    from hip_decisions import hip_decisions
    net, ref = _joint_nets(75, dropout_keep_prob=1.0, dtype="bf16")
    ref.conv_multiply = "bf16"
    batches = _joint_batches(3, 8, 700)
    for k, batch in enumerate(batches, 1):
        lr = step_lr(1e-3, k)
        assert net.step == k - 1
        sync_oracle_from_net(net, ref, k - 1)
        ref.z_pivots = _pivots(net) if k > 1 else None      # (first step: the moving mean, on both sides)
        if k > 1:
            moved = max(float((p - ref.p[sc + "/BatchNorm/moving_mean"]).abs().max()) for sc, p in ref.z_pivots.items())
            assert moved > 0, "the pivots are still the moving means"
        net.train_step(_device(batch), lr)
        torch.cuda.synchronize()
        logits = net.logits.detach().cpu().numpy()
        grads = net.grads_state_dict()
        ref.z_storage_bf16 = {sc for l in net.image.layers if l.z16 for (sc, _, _) in l.scopes}
        assert len(ref.z_storage_bf16) >= 30
        ref.inject = hip_decisions(net)
        out = ref.train_step(batch, lr)
        dl = float(np.abs(logits - out["logits"].numpy()).max())
        dloss = abs(net.total_loss_value() - out["loss"])
        rels = sorted((float(np.linalg.norm(grads[n].reshape(g.shape) - g.numpy()) / max(float(g.norm()), 1e-30)), n)
                      for n, g in out["grads"].items())
        print("joint/bf16 step %d vs the bf16-emulating oracle: max|dlogits| %.3e (gate 5e-2), |dloss| %.3e (1e-2), gradient "
              "relative L2 median %.3e (0.2), worst %.3e (%s)" % (k, dl, dloss, rels[len(rels) // 2][0], rels[-1][0], rels[-1][1]))
        assert dl <= 5e-2 and dloss <= 1e-2 and rels[len(rels) // 2][0] <= 0.2, "step %d: %r" % (k, (dl, dloss, rels[len(rels) // 2]))
    assert net.step == 3


# ---- the checks above can fail ------------------------------------------------------------------------------------------

PLANTED_LR0 = 4e-3      # steps of 4e-3, 2e-3: see the margins in the docstrings below
VARIABLE_CHECK = r"^step 2: (Text/rnn/|W_softmax|b_softmax)"      # _check_step's post-step variable asserts name the variable


def test_planted_stale_winograd_filter_is_caught_at_step_two():
    """Configuration 2 with ConvBN._refresh_weights turned into a no-op after step 1 for Mixed_5c/Branch_1/Conv2d_0b_3x3
    (trainable, Winograd: the layer keeps the G g G^T of the step-1 weights in forward and dgrad).  Step 1 must pass, step
    2 must raise.  Oracle alone on the CPU, same parameters and batches (lr 1e-3 at step 1, as here): evaluating step 2's
    forward with this layer's filter one Adam step old moves the logits by 1.25e-1, 125x the 1e-3 logits gate (the
    ReLU decisions move with them, so the guard on the injected decisions may be the gate that speaks first)."""
    net, ref = _joint_nets(71)
    state = {}

    def plant(k):
        if k == 1:
            lay = [l for l in net.image.layers if l.trainable and l.k == 3 and l.cout == 384]
            assert len(lay) == 1 and lay[0].fwd.u is not None, "no prepared filter form to go stale"
            lay[0]._refresh_weights = lambda: None
        state["last"] = k

    with pytest.raises(AssertionError, match=r"^step 2: "):
        free_run(net, ref, _joint_batches(2, 4, 100), 1e-3, "planted/stale-filter", hip_mask=True, grad_tol=2e-3,
                 after_step=plant)
    assert state["last"] == 1


def test_planted_stuck_step_counter_is_caught_at_step_two():
    """Text steps whose lr_t is always computed with t = 1 (the step count the net shows stays right, so only the
    variable check can notice).  lr_t / lr = sqrt(1 - b2^t) / (1 - b1^t): 0.316 at t = 1, 0.235 at t = 2.  Oracle alone on
    the CPU, same parameters and batches, step 2 at lr 2e-3 with either t: the well-resolved entries of the four variables
    differ by 5.1e-4 .. 5.9e-4 in the median (51x the 1e-5 gate), 87 .. 92 % of them by more than 1e-4, and 0 .. 3.6 % stay
    within 1e-5 where the gate wants 99 %.  (At lr 1e-3 the median would be 8x the gate only: hence PLANTED_LR0.)"""
    V, D, H, T, B = TEXT_DIMS["small"]
    net, ref = _text_nets(V, D, H, T, seed=81)
    orig = net.train_step

    def stuck(batch, lr, dropout_mask=None, seed=None):
        shown = net.step
        net.step = 0
        try:
            return orig(batch, lr, dropout_mask=dropout_mask, seed=seed)
        finally:
            net.step = shown + 1

    net.train_step = stuck
    batches = [step_batch(k, B, T, V, 200, False) for k in range(1, 3)]
    with pytest.raises(AssertionError, match=VARIABLE_CHECK):
        free_run(net, ref, batches, PLANTED_LR0, "planted/stuck-step")


def test_planted_stale_device_lr_is_caught_at_step_two():
    """Captured text steps whose graph keeps reading step 1's lr_t: after step 1 the net's `lr_t_dev` attribute points at
    another (valid) device word, so train_step's fill_ no longer reaches the one the capture baked in.  Oracle alone on
    the CPU, same parameters and batches, step 2 with lr_t(t = 1, 4e-3) in place of lr_t(t = 2, 2e-3), a 2.7x step: the
    well-resolved entries differ by 2.6e-3 .. 3.1e-3 in the median (260x the 1e-5 gate), 96 .. 100 % of them by more than
    1e-4, and at most 0.2 % stay within 1e-5."""
    from hip_decisions import keep_activations
    V, D, H, T, B = TEXT_DIMS["small"]
    net, ref = _text_nets(V, D, H, T, seed=83)
    batches = [step_batch(k, B, T, V, 500, False) for k in range(1, 3)]
    keep_activations(net)
    dev = _device(batches[0])
    assert net.capture_step(dev)
    baked = net.lr_t_dev      # kept alive: the graph reads it

    def plant(k):
        if k == 1:
            net.lr_t_dev = torch.zeros_like(baked)

    with pytest.raises(AssertionError, match=VARIABLE_CHECK):
        free_run(net, ref, batches, PLANTED_LR0, "planted/stale-lr_t_dev", dev=dev, after_step=plant)
    assert net._graph is not None and baked.numel() == 1
