#!/usr/bin/env python3
"""HBM bytes per decode layer from a rocprofv3 --pmc FETCH_SIZE pass over bench.py's decode-layer
line (run with --full --no-other-mode --ramp-s 0).

Every dispatch of the layer pass counts, whatever its kernel is called (an
allow-list of kernel names missed the round-5 gate/up kernel and published half the bytes).  The
dispatches are taken in dispatch order; each attention dispatch (``attn_decode``: one per layer)
marks a layer, whose window runs from the dispatch just before it (the q/k/v launch) to the
dispatch before the next layer's q/k/v launch; the last layer's window is as long as the others.
The windows of the timed graph-replayed passes must share one shape (>= 80 % of all windows: the
eager warm-up pass, which also runs the layer's host-side torch ops, is reported and left out) of
at least five dispatches — q/k/v, the attention, o, gate/up, down — with the attention second and
GEMV kernels in the other four places; otherwise the tool fails.

bytes per layer = mean over the windows of sum(FETCH_SIZE x 1024 x 2) (the gfx950 correction,
MI355X_MICROARCH.md HBM section).
Usage: python tools/decode_traffic.py <pmc dir> <out.json>"""
import collections
import csv
import glob
import json
import os
import sys

CLASSES = ("qkv_norm", "attention", "o_residual", "gate_up_norm_silu", "down_residual")

def _marker(name):
    return "attn_decode" in name


def _classes(rows):
    return CLASSES, 1  # (classes, the attention's place in a layer)


def _rows(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        for i, r in enumerate(csv.DictReader(open(f))):
            if r.get("Counter_Name") != "FETCH_SIZE":
                continue
            key = (int(r["Dispatch_Id"]) if r.get("Dispatch_Id", "").isdigit()
                   else int(r.get("Start_Timestamp") or i))
            rows.append((key, r.get("Kernel_Name", ""), float(r["Counter_Value"]) * 1024 * 2))
    rows.sort(key=lambda t: t[0])
    return rows


def layer_windows_all(rows):
    att = [i for i, r in enumerate(rows) if _marker(r[1])]
    return collections.Counter((att[j + 1] - att[j]) for j in range(len(att) - 1))


def layer_windows(rows):
    """[(names, bytes)] per layer window (see the module docstring); raises SystemExit when the
    pass does not have the decode layer's shape."""
    classes, at = _classes(rows)
    att = [i for i, r in enumerate(rows) if _marker(r[1])]
    if len(att) < 2:
        raise SystemExit("fewer than two attention dispatches: not a decode-layer pass")
    if att[0] < at:
        raise SystemExit("no q/k/v dispatch before the first attention dispatch")
    spans = [att[j + 1] - att[j] for j in range(len(att) - 1)]
    width = collections.Counter(spans).most_common(1)[0][0]
    wins = []
    for j, a in enumerate(att):
        end = att[j + 1] - at if j + 1 < len(att) else a - at + width
        if end > len(rows):
            raise SystemExit(f"last layer window runs past the pass ({end} > {len(rows)})")
        wins.append(rows[a - at:end])
    shapes = collections.Counter(len(w) for w in wins)
    n, count = shapes.most_common(1)[0]
    # the graph-replayed passes (bench.py's timed decode line) are the bulk of the windows; the
    # one eager warm-up pass before the capture also runs the layer's host-side torch ops (mask /
    # position tensors), which are not part of the replayed step: those windows are reported and
    # left out, never mixed in
    if count < 0.8 * len(wins):
        raise SystemExit(f"layer windows of different lengths {dict(shapes)}: no dominant decode "
                         "pass (run bench.py with --full --no-other-mode)")
    wins = [w for w in wins if len(w) == n]
    if n < len(classes):
        raise SystemExit(f"{n} dispatches per layer: fewer than the {len(classes)} kernel classes "
                         f"{classes} (five kernel classes)")
    for w in wins:
        names = [r[1] for r in w]
        if not _marker(names[at]) or any("gemv" not in names[p] for p in range(len(classes))
                                         if p != at):
            raise SystemExit(f"unexpected layer window {names}")
    return wins


def main():
    d, out = sys.argv[1:3]
    rows = _rows(d)
    if not rows:
        raise SystemExit(f"no FETCH_SIZE rows under {d}")
    all_wins = layer_windows_all(rows)
    wins = layer_windows(rows)
    n = len(wins[0])
    classes, _ = _classes(rows)
    per_pos = [[w[p][2] for w in wins] for p in range(n)]
    cls = list(classes) + [f"extra_{p}" for p in range(len(classes), n)]
    total = sum(sum(r[2] for r in w) for w in wins) / len(wins)
    res = {"workload": "decode_layer_int4_g128", "layers_dispatched": len(wins),
           "dispatches_per_layer": n,
           "fetch_bytes_per_launch": total,
           "fetch_bytes_per_layer": total,
           "per_class_mean_bytes": {c: sum(v) / len(v) for c, v in zip(cls, per_pos)},
           "per_class_kernel": {c: wins[-1][p][1][:160] for p, c in enumerate(cls)},
           "kernel_classes": n,
           "window_lengths_seen": {str(k): v for k, v in sorted(all_wins.items())},
           "correction": "FETCH_SIZE KiB x 1024 x 2 (gfx950 counts half of wide streaming reads)",
           "method": ("every dispatch of each layer window (the q/k/v dispatch before an attention "
                      "dispatch up to the next layer's q/k/v), dispatch order; mean over windows"),
           "source": "rocprofv3 --pmc FETCH_SIZE, separate pass, bench.py --full --no-other-mode",
           "excluded": ("windows of another length (the eager warm-up pass before the graph "
                        "capture, which also runs host-side torch ops)")}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
