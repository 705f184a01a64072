#!/usr/bin/env python3
"""Which step's kernels run on which hardware queue, and when (run ON the GPU box): the streaming bench line under
`rocprofv3 --kernel-trace` (nothing else in the profiler run, the program directly behind `--`), condensed to one row per step.

A step's launches are recognised by the search walk's grid: the first chunk of an alignment (eight iterations) walks every scan of the
batch, the later chunks only the scans still open (gn_driver.hip, enqueue_chunk) — and every step of the bench aligns the same scans,
so the sequence of grids is the same for every step. On one queue the launches of a step therefore read [full x 8][part ...]; two
first chunks back to back with no partial launches between them are two alignments in flight on ONE in-order stream.

    python3 tools/queue_trace.py [--steps 80] [--window 12] [--save-csv FILE] [--out profiles/....txt] [--lib liblocgpu.so]
    python3 tools/queue_trace.py --csv FILE            # condense a trace that was saved earlier (no GPU needed)
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collect(a):
    d = tempfile.mkdtemp(prefix="locgpu_queue_trace_", dir="/tmp")
    try:
        env = dict(os.environ, TMPDIR="/tmp")
        if a.lib:
            env["LOCGPU_LIB"] = os.path.abspath(a.lib)
        cmd = ["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               os.path.realpath(sys.executable), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)] + a.bench_args
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
        if r.returncode != 0:
            raise SystemExit("bench.py under rocprofv3 failed (%d): %s" % (r.returncode, r.stderr[-800:]))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
        f = glob.glob(os.path.join(d, "**", "t_kernel_trace.csv"), recursive=True)[0]
        if a.save_csv:
            os.makedirs(os.path.dirname(os.path.abspath(a.save_csv)), exist_ok=True)
            shutil.copy(f, a.save_csv)
        return list(csv.DictReader(open(f))), (line[-1] if line else None)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def condense(rows, window):
    """rows of a kernel trace → lines of text."""
    ev = []
    for q in rows:
        size = int(q["Grid_Size_X"]) * int(q["Grid_Size_Y"]) * int(q["Grid_Size_Z"])
        ev.append(dict(q=q["Queue_Id"], t0=int(q["Start_Timestamp"]), t1=int(q["End_Timestamp"]), walk="icp_search_walk_kernel" in q["Kernel_Name"], size=size))
    ev.sort(key=lambda e: e["t0"])
    full = max(e["size"] for e in ev if e["walk"])
    # chunks per queue: a run of consecutive iterations whose walk has the same grid; every launch belongs to the walk in front of it
    chunks = []
    for qid in sorted({e["q"] for e in ev}):
        cur = None
        for e in (x for x in ev if x["q"] == qid):
            if e["walk"]:
                if cur is None or cur["size"] != e["size"] or (cur["size"] == full and cur["iters"] == 8):
                    cur = dict(q=qid, size=e["size"], iters=0, t0=e["t0"], t1=e["t1"], busy=0)
                    chunks.append(cur)
                cur["iters"] += 1
            if cur is not None:
                cur["t1"] = max(cur["t1"], e["t1"])
                cur["busy"] += e["t1"] - e["t0"]
    # steps: every full chunk opens one; the partial chunks behind it on its queue go to the oldest step of the queue that has not had
    # a chunk of that place yet (an alignment's chunks keep their order, and its second chunk has the largest partial grid)
    part_sizes = sorted({c["size"] for c in chunks if c["size"] != full}, reverse=True)
    second = part_sizes[0] if part_sizes else None
    steps, open_q = [], {}
    for c in sorted(chunks, key=lambda c: c["t0"]):
        lst = open_q.setdefault(c["q"], [])
        if c["size"] == full:
            st = dict(q=c["q"], first=c, late=[], behind=bool(lst and not lst[-1]["late"]))
            steps.append(st)
            lst.append(st)
        elif lst:
            if c["size"] == second:
                while len(lst) > 1 and lst[0]["late"]:
                    lst.pop(0)
            lst[0]["late"].append(c)
    steps.sort(key=lambda s: s["first"]["t0"])
    for i, s in enumerate(steps):
        s["i"] = i
    # spans in which no first chunk runs on any queue: only the small launches of late chunks (or nothing)
    iv = sorted((s["first"]["t0"], s["first"]["t1"]) for s in steps)
    gaps, end = [], iv[0][1]
    for t0, t1 in iv[1:]:
        if t0 > end:
            gaps.append((end, t0))
        end = max(end, t1)
    n = len(steps)
    lo = max(0, n // 2 - window // 2)
    win = steps[lo:lo + window]
    base = win[0]["first"]["t0"]
    ms = lambda t: (t - base) / 1e6
    out = []
    body = steps[n // 4:]  # steady state: the warm-up and the pipeline's fill are in the first quarter
    span = (body[-1]["first"]["t0"] - body[0]["first"]["t0"]) / 1e6 / max(len(body) - 1, 1)
    out.append("steps seen %d on queues %s; %.2f ms between the starts of consecutive steps (last %d steps)" % (n, sorted({s["q"] for s in steps}), span, len(body)))
    out.append("steps whose first chunk was queued directly behind another step's first chunk on the same queue: %d of %d" % (sum(s["behind"] for s in body), len(body)))
    bg = [(a, b) for a, b in gaps if a >= body[0]["first"]["t0"]]
    long_gaps = [(a, b) for a, b in bg if b - a >= 0.5e6]
    out.append("spans without any first-chunk kernel (late chunks only): %d of >= 0.5 ms, %.2f ms in all = %.3f ms per step; all spans %.3f ms per step"
               % (len(long_gaps), sum(b - a for a, b in long_gaps) / 1e6, sum(b - a for a, b in long_gaps) / 1e6 / len(body), sum(b - a for a, b in bg) / 1e6 / len(body)))
    # how many queues have a kernel running, over the steady part of the run (a sweep over the dispatches' edges)
    w0, w1 = body[0]["first"]["t0"], body[-1]["first"]["t0"]
    edges = []
    for qid in sorted({e["q"] for e in ev}):
        end = None
        for e in (x for x in ev if x["q"] == qid and x["t1"] > w0 and x["t0"] < w1):  # a queue runs its kernels in order: merge them into busy intervals
            t0, t1 = max(e["t0"], w0), min(e["t1"], w1)
            if end is not None and t0 <= end:
                if t1 > end:
                    edges[-1] = (t1, -1, qid)
                    end = t1
                continue
            edges += [(t0, 1, qid), (t1, -1, qid)]
            end = t1
    hist, per_q, level, last = {}, {}, 0, w0
    for t, d, qid in sorted(edges):
        hist[level] = hist.get(level, 0) + t - last
        level, last = level + d, t
        per_q[qid] = per_q.get(qid, 0) + (-t if d > 0 else t)
    hist[level] = hist.get(level, 0) + w1 - last
    out.append("queues with a kernel running, share of the time: " + ", ".join("%d: %.1f %%" % (k, 100.0 * v / (w1 - w0)) for k, v in sorted(hist.items())))
    out.append("busy share of each queue: " + ", ".join("q%s %.1f %%" % (k, 100.0 * v / (w1 - w0)) for k, v in sorted(per_q.items())))
    out.append("")
    out.append("| step | queue | first chunk [ms] | late chunks [ms] (walk grid / iterations) | queued behind |")
    out.append("|---|---|---|---|---|")
    for s in win:
        late = "; ".join("%.2f-%.2f (%d / %d)" % (ms(c["t0"]), ms(c["t1"]), c["size"] * 256 // full, c["iters"]) for c in s["late"]) or "-"
        out.append("| %d | %s | %.2f-%.2f | %s | %s |" % (s["i"], s["q"], ms(s["first"]["t0"]), ms(s["first"]["t1"]), late, "step %d's first chunk" % (s["i"] - 1) if s["behind"] else ""))
    out.append("")
    out.append("spans of the window without a first-chunk kernel: " + (", ".join("%.2f-%.2f" % (ms(a), ms(b)) for a, b in gaps if win[0]["first"]["t0"] <= a <= win[-1]["first"]["t1"] and b - a >= 0.2e6) or "none of >= 0.2 ms"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=int, default=12, help="steps in the table, from the middle of the run")
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--lib", default=None, help="LOCGPU_LIB of the run")
    ap.add_argument("--csv", default=None, help="condense this kernel trace instead of running the bench")
    ap.add_argument("--save-csv", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("bench_args", nargs="*", help="further bench.py arguments (behind --)")
    a = ap.parse_args()
    if a.csv:
        rows, line = list(csv.DictReader(open(a.csv))), None
    else:
        rows, line = collect(a)
    out = condense(rows, a.window)
    if line:
        out.insert(0, "bench line under the profiler: " + line[:160])
    text = "\n".join(out)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
