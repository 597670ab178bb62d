"""num_clones without a device: the config check of the front ends, the deferred mode of the gradient reducer (world 2 over
gloo on CPU tensors, as tests/test_dp_cpu.py) and the argument errors of ds_grad_accumulate, which are reported before any
launch."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tumblr_emotions_amd.training import check_clones_config


def test_num_clones_config_check():
    assert check_clones_config({}) == 1
    for k in (1, 2, 8):
        assert check_clones_config({"num_clones": k}) == k
    for bad in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="num_clones"):
            check_clones_config({"num_clones": bad})
    with pytest.raises(ValueError, match="sync_bn"):
        check_clones_config({"num_clones": 2, "sync_bn": True})
    for dtype in ("bf16", "f16"):
        with pytest.raises(NotImplementedError, match="dtype"):
            check_clones_config({"num_clones": 2, "dtype": dtype})
    # one clone: neither key is this check's business
    assert check_clones_config({"num_clones": 1, "sync_bn": True, "dtype": "bf16"}) == 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    from tumblr_emotions_amd import dp
    from tumblr_emotions_amd.dp import GradientReducer
    from tumblr_emotions_amd.params import ParamStore
    dp.init_distributed("gloo", rank=rank, world_size=world)
    try:
        st = ParamStore("cpu")
        st.declare("conv/weights", (3, 5), True, l2=True, bucket=1)
        st.declare("head/W", (7,), True, bucket=1)
        st.declare("upstream/beta", (6,), True, bucket=2)
        st.finalize()
        assert st.n_bucket1 == 24 and st.n_trainable_padded == 32
        mine = torch.arange(32, dtype=torch.float32) * (rank + 1)
        st.grad.copy_(mine)
        red = GradientReducer(st.grad, st.n_bucket1, overlap=True)
        red.expect("a", "b")
        # deferred: the stages report, nothing is recorded, launched or reduced
        red.begin_step(defer=True)
        red.stage_done("a")
        red.stage_done("b")
        assert red._pending is None and not red._ready and not red._events
        assert torch.equal(st.grad, mine)
        assert red.finish() == 0.5
        assert torch.equal(st.grad, torch.arange(32, dtype=torch.float32) * 3)      # both buckets, element-wise sum
        # a following plain step behaves as before
        st.grad.copy_(mine)
        red.begin_step()
        red.stage_done("a")
        red.stage_done("b")
        assert red._ready == {"a", "b"}
        assert red.finish() == 0.5
        assert torch.equal(st.grad, torch.arange(32, dtype=torch.float32) * 3)
        out.put(rank)
    finally:
        dist.destroy_process_group()


def test_deferred_reducer_reduces_both_buckets_in_finish():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0, "rank failed (exit code %r)" % p.exitcode
    assert sorted(out.get(timeout=10) for _ in range(2)) == [0, 1]


def test_grad_accumulate_argument_errors_are_reported_before_any_launch():
    from tumblr_emotions_amd import _lib
    lib = _lib.load()
    buf = C.c_void_p(1 << 20)      # a 16-byte aligned address that is never dereferenced: every case fails its argument check
    cases = [(None, buf, 4, 0), (buf, None, 4, 0), (None, None, 4, 0), (buf, buf, 6, 0), (buf, buf, 4, 3)]
    for acc, g, n, mode in cases:
        assert lib.ds_grad_accumulate(acc, g, n, mode, None) == -1, (acc, g, n, mode)
        assert "ds_grad_accumulate" in lib.ds_last_error().decode()
