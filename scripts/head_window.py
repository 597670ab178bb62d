#!/usr/bin/env python
"""The head window of a step, from a rocprofv3 kernel trace (rocpd sqlite): the stretch between the end of
avgpool_dropout_fwd (Mixed_5c's forward is through) and the start of avgpool_dropout_bwd (Mixed_5c's backward may begin).
Prints the window's wall time, the dispatches that START inside it (name, start, duration), how many of them there are,
and where lstm_seq_bwd starts -- for the last `steps` full steps (between two adam_tf_kernel launches).
    python scripts/head_window.py x_results.db [steps]"""
import re
import sqlite3
import sys


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n)
    return re.sub(r"\(.*", "", n)[:64]


def main():
    cur = sqlite3.connect(sys.argv[1]).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    ncol = "name" if "name" in cols else "kernel_name"
    rows = sorted(cur.execute("select start, end, %s from kernels" % ncol).fetchall())
    adam = [i for i, r in enumerate(rows) if "adam_tf" in r[2]]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for back in range(min(steps, len(adam) - 1), 0, -1):
        seg = rows[adam[-1 - back] + 1:adam[-back] + 1]
        t0 = seg[0][0]
        fwd = [r for r in seg if "avgpool_dropout_fwd" in r[2]]
        bwd = [r for r in seg if "avgpool_dropout_bwd" in r[2]]
        if not fwd or not bwd:
            print("step -%d: no avgpool_dropout_fwd / _bwd in the step" % back)
            continue
        w0, w1 = fwd[0][1], bwd[0][0]
        inside = [r for r in seg if w0 <= r[0] < w1]
        lstm = [r for r in seg if "lstm_seq_bwd" in r[2]]
        print("step -%d: %d kernels, wall %.3f ms; avgpool_dropout_fwd ends %.3f, avgpool_dropout_bwd starts %.3f: "
              "window %.3f ms, %d dispatches start inside, their kernel time %.3f ms; lstm_seq_bwd starts %s"
              % (back, len(seg), (max(r[1] for r in seg) - t0) / 1e6, (w0 - t0) / 1e6, (w1 - t0) / 1e6, (w1 - w0) / 1e6,
                 len(inside), sum(r[1] - r[0] for r in inside) / 1e6,
                 "%.3f" % ((lstm[0][0] - t0) / 1e6) if lstm else "n/a"))
        if back == 1:
            for s, e, n in inside:
                print("  %8.3f  %6.1f us  %s" % ((s - t0) / 1e6, (e - s) / 1e3, short(n)))


if __name__ == "__main__":
    main()
