"""How far does the frozen-BatchNorm reference step in fp32 sit from itself in fp64 along the SAME decisions?  (CPU only.)

The step tests of tests/test_frozen_bn_gpu.py compare the HIP step with the fp64 reference along the HIP path's ReLU / pool
decisions at the project's gates (logits and loss 1e-3, every gradient 1e-3 relative L2 and max-norm, TF-Adam 1e-5 on the
resolved entries).  Those gates are only fair if ANY fp32 evaluation can meet them on these inputs, so this script measures
the reference against itself: the decisions are recorded from the fp64 run and injected into an fp32 and an fp64 run.
DESIGN.md 7.9 records the figures.

The inputs and the reference subclass are the TESTS' own (`_inputs` of tests/test_frozen_bn_gpu.py, `FrozenBNRef` of
tests/test_frozen_bn_cpu.py, imported with tests/ on sys.path), so that the spread is measured on exactly what the tests
compare: when those helpers change, the figures recorded in DESIGN.md change with them and this script has to be run again.

usage: python scripts/frozen_bn_oracle_spread.py [--out profiles/frozen_bn_oracle_spread.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(mode, B):
    from test_frozen_bn_gpu import _inputs
    from test_frozen_bn_cpu import FrozenBNRef
    params, emb, batch, mask = _inputs(mode, B)
    rec = FrozenBNRef(params, emb, mode, torch.float64)
    rec.record = {}
    with torch.no_grad():
        rec.forward(batch, torch.tensor(mask))
    runs = {}
    for dt in (torch.float64, torch.float32):
        ref = FrozenBNRef(params, emb, mode, dt)
        ref.inject = rec.record
        out = ref.train_step(batch, 1e-3, torch.tensor(mask).to(dt))
        runs[dt] = (ref, out)
    (r64, o64), (r32, o32) = runs[torch.float64], runs[torch.float32]
    rel = emax = 0.0
    adam = 1.0
    for name, g in o64["grads"].items():
        g = g.numpy()
        d = o32["grads"][name].double().numpy() - g
        rel = max(rel, np.linalg.norm(d) / max(np.linalg.norm(g), 1e-30))
        emax = max(emax, np.abs(d).max() / max(np.abs(g).max(), 1e-30))
        big = np.abs(g) > 1e-2 * max(np.abs(g).max(), 1e-12)
        dw = np.abs(r32.p[name].detach().double().numpy() - r64.p[name].detach().numpy())
        adam = min(adam, float((dw[big] <= 1e-5).mean()))
    return dict(mode=mode, B=B, logits=float((o32["logits"].double() - o64["logits"]).abs().max()),
                logits_max=float(o64["logits"].abs().max()), loss=abs(o32["loss"] - o64["loss"]),
                grad_rel_l2=float(rel), grad_max_norm=float(emax), adam_share_within_1e5=adam)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = [spread("joint", 4), spread("image", 2)]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
