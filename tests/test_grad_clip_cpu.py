"""Gradient clipping and the non-finite guard, the parts that need no device: the segment and chunk tables
that ParamStore.finalize() builds for ds_grad_norms / ds_adam_tf_clipped, and the refused configurations."""
import numpy as np
import pytest

from grad_clip_ref import flat_indices


@pytest.fixture(scope="module")
def joint_store():
    """The joint model's parameter store, declared by the real engines on the CPU (finalize() allocates host tensors)."""
    from tumblr_emotions_amd.engine_image import InceptionV1Engine
    from tumblr_emotions_amd.engine_text import JointHeadEngine, TextTowerEngine
    from tumblr_emotions_amd.params import ParamStore
    st = ParamStore(device="cpu")
    InceptionV1Engine(st, 256, 224, 0.8, True, "cpu")
    TextTowerEngine(st, 51, 20, 32, 10, "cpu")
    JointHeadEngine(st, 256, 32, 512, 15, "cpu")
    st.finalize()
    return st


def _check_tables(names, seg, chunks, entries, n, chunk):
    """Every flat element of [0, n) is in exactly one chunk; the elements of a variable are exactly its segment's; pads are
    exactly what no variable owns; no chunk straddles a segment; a segment's chunks are consecutive and in order."""
    assert seg.dtype == np.int64 and chunks.dtype == np.int64 and seg.shape == (len(names), 8) and chunks.shape[1] == 4
    owner = np.full(n, -2, np.int64)                 # -2: not visited, -1: pad, s: segment
    for c, (s, k0, count, _) in enumerate(chunks):
        assert 0 < count <= chunk or (s == -1 and 0 < count), (c, count)
        if s == -1:
            idx = np.arange(k0, k0 + count)
        else:
            off, rows, ld, c0, ncols, first, nch, _ = seg[s]
            assert first <= c < first + nch and k0 == (c - first) * chunk and k0 + count <= rows * ncols, c
            idx = flat_indices(seg[s], k0, count)
        assert idx.min() >= 0 and idx.max() < n
        assert (owner[idx] == -2).all(), "chunk %d visits an element twice" % c
        owner[idx] = s
    assert (owner != -2).all(), "an element no chunk visits"
    for s, row in enumerate(seg):
        off, rows, ld, c0, ncols, first, nch, _ = row
        assert nch == -(-rows * ncols // chunk) and (chunks[first:first + nch, 0] == s).all()
        assert int((owner == s).sum()) == rows * ncols
    want = np.full(n, -1, np.int64)                  # from the entries themselves
    s = 0
    for e in entries:
        view = want[e.offset:e.offset + e.numel].reshape(-1, e.shape[-1])
        for (name, c0, c1) in (e.columns or [(e.name, 0, e.shape[-1])]):
            assert names[s] == name
            view[:, c0:c1] = s
            s += 1
    assert s == len(names) and np.array_equal(owner, want)


def test_tables_of_the_joint_model_partition_the_flat_buffer(joint_store):
    from tumblr_emotions_amd.params import CLIP_CHUNK
    st = joint_store
    tr = sorted((e for e in st.entries.values() if e.trainable), key=lambda e: e.offset)
    n = st.theta.numel()
    _check_tables(st.clip_names, st.clip_segments, st.clip_chunks, tr, n, CLIP_CHUNK)
    trainable_tf_names = [n_ for e in st.entries.values() if e.trainable for n_ in ([c[0] for c in e.columns] if e.columns else [e.name])]
    assert sorted(st.clip_names) == sorted(trainable_tf_names) and len(set(st.clip_names)) == len(st.clip_names)
    assert set(st.clip_names) <= set(st.tf_names())
    # the fused block-input tensor of Mixed_5c: three names, three segments over ONE offset, disjoint column ranges
    fused = [e for e in tr if e.columns and len(e.columns) > 1 and len(e.shape) == 4]
    assert len(fused) == 1 and len(fused[0].columns) == 3 and all("Mixed_5c" in c[0] for c in fused[0].columns)
    rows = [st.clip_segments[st.clip_names.index(name)] for (name, _, _) in fused[0].columns]
    assert all(r[0] == fused[0].offset and r[2] == fused[0].shape[-1] and r[1] == fused[0].numel // fused[0].shape[-1] for r in rows)
    assert [(r[3], r[3] + r[4]) for r in rows] == [(c0, c1) for (_, c0, c1) in fused[0].columns]
    assert sum(r[1] * r[4] for r in rows) == fused[0].numel
    # pads are few: the padding of the odd-sized biases
    pads = st.clip_chunks[st.clip_chunks[:, 0] == -1]
    assert int(pads[:, 2].sum()) == n - st.n_trainable
    seg_dev, chunk_dev = st.clip_tables()
    assert seg_dev.device.type == "cpu" and np.array_equal(seg_dev.numpy(), st.clip_segments)
    assert np.array_equal(chunk_dev.numpy(), st.clip_chunks)


def test_tables_of_a_hand_made_store_with_pads_and_columns():
    """The layout of the kernel tests: odd sizes (pads), sizes around the chunk, a fused tensor -- with a small chunk, so
    that a column segment spans several chunks that start in the middle of a row."""
    from tumblr_emotions_amd.params import ParamStore, build_clip_tables
    st = ParamStore(device="cpu")
    st.declare("a", (1,), True, l2=True)
    st.declare("b", (3,), True, l2=True)
    st.declare("frozen", (7,), False)
    st.declare("fused", (1, 1, 5, 12), True, columns=[("f0", 0, 5), ("f1", 5, 6), ("f2", 6, 12)])
    st.declare("c", (17,), True, bucket=2)
    st.finalize()
    tr = sorted((e for e in st.entries.values() if e.trainable), key=lambda e: e.offset)
    assert st.clip_names == ["a", "b", "f0", "f1", "f2", "c"]
    for chunk in (4, 7, 4096):
        names, seg, chunks = build_clip_tables(tr, st.theta.numel(), chunk)
        _check_tables(names, seg, chunks, tr, st.theta.numel(), chunk)
    assert st.theta.numel() == 4 + 4 + 60 + 20 and int((st.clip_chunks[:, 0] == -1).sum()) == 3


def test_refused_configurations_need_no_device():
    from tumblr_emotions_amd.net import check_clip_config
    from tumblr_emotions_amd import ops
    from tumblr_emotions_amd.training import clip_net_kwargs
    assert check_clip_config() == (ops.CLIP_NONE, 0.0)
    assert check_clip_config(clip_gradient_norm=2) == (ops.CLIP_PER_VARIABLE, 2.0)
    assert check_clip_config(clip_global_norm=np.float32(0.5)) == (ops.CLIP_GLOBAL, 0.5)
    with pytest.raises(ValueError, match="mutually exclusive"):
        check_clip_config(clip_gradient_norm=1.0, clip_global_norm=1.0)
    for key in ("clip_gradient_norm", "clip_global_norm"):
        for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True, [1.0]):
            with pytest.raises(ValueError, match="finite number > 0"):
                check_clip_config(**{key: bad})
            with pytest.raises(ValueError, match="finite number > 0"):
                clip_net_kwargs({key: bad})
    assert clip_net_kwargs({}) == {} and clip_net_kwargs({"clip_global_norm": None}) == {}
    assert clip_net_kwargs({"clip_global_norm": 3.0, "skip_nonfinite_steps": True, "log_gradient_norms": True}) == {
        "clip_global_norm": 3.0, "skip_nonfinite_steps": True}
    with pytest.raises(ValueError, match="mutually exclusive"):
        clip_net_kwargs({"clip_gradient_norm": 1.0, "clip_global_norm": 1.0})
    with pytest.raises(ValueError, match="log_gradient_norms"):
        clip_net_kwargs({"log_gradient_norms": True})
    with pytest.raises(ValueError, match="must be a bool"):
        clip_net_kwargs({"skip_nonfinite_steps": 1})


def test_the_model_constructor_refuses_before_it_asks_for_a_device():
    """SentimentNet checks the clipping arguments first: the ValueError comes also where there is no GPU to build on."""
    from tumblr_emotions_amd.net import SentimentNet
    with pytest.raises(ValueError, match="mutually exclusive"):
        SentimentNet(mode="text", clip_gradient_norm=1.0, clip_global_norm=2.0)
    for bad in (0, -3.0, float("nan"), "big"):
        with pytest.raises(ValueError, match="finite number > 0"):
            SentimentNet(mode="text", clip_global_norm=bad)
        with pytest.raises(ValueError, match="finite number > 0"):
            SentimentNet(mode="text", clip_gradient_norm=bad)
