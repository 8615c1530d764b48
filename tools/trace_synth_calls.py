"""zkw_ram_synthesize call by call, from `rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -- python bench.py
--gpus 1 --blocks 2000 --steps 1 --warmup 1 --pipelines 1 ...`: first start to last end, the sum of the kernel durations, the duration of and
the gap in front of each kernel, the memset and the copy (docs/KERNELS.md 3.3 "Round 17"). usage: trace_synth_calls.py DIR LABEL"""
import csv, glob, sys, statistics as st
d, tag = sys.argv[1], sys.argv[2]
kf = glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True)[0]
mf = glob.glob(f"{d}/**/*memory_copy_trace.csv", recursive=True)
rows = list(csv.DictReader(open(kf)))
def short(n):
    for k in ("k_gather_encode", "k_ram_nd_tiles", "k_ram_nd_scan", "k_ram_fill_poseidon", "k_ram_fill_C", "k_ram_fill_D", "k_ram_fill_tail"):
        if k in n:
            if k == "k_ram_fill_poseidon":
                return k + ("<0>" if "ILi0E" in n else "<1>" if "ILi1E" in n else "")
            return k
    if "fillBuffer" in n or "FillBuffer" in n: return "memset"
    if "copyBuffer" in n: return "copy (job table)"
    return None
ev = []
for r in rows:
    s = short(r["Kernel_Name"])
    if s: ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, r.get("Queue_Id"), r.get("Stream_Id")))
ev.sort()
copies = []
for f in mf:
    for r in csv.DictReader(open(f)):
        copies.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")))
copies.sort()
# calls: from a k_gather_encode (and the memset / copy just before the next kernel) to the last k_ram_fill_* before the next gather on that queue
calls, cur = [], None
for e in ev:
    if e[2] == "k_gather_encode":
        if cur: calls.append(cur)
        cur = [e]
    elif cur is not None and e[2] not in ("memset", "copy (job table)"):
        cur.append(e)
    elif cur is not None and not any(x[2].startswith("k_ram") for x in cur):  # the memset and the copy of a call come before its first k_ram_* kernel
        cur.append(e)
if cur: calls.append(cur)
names = {}
warm = []
for c in calls:
    ks = [e for e in c]
    if len(ks) < 3: continue
    warm.append(c)
# drop the first tenth (cold slots, first launches)
warm = warm[len(warm) // 10:]
import collections
gap, dur, cnt = collections.defaultdict(list), collections.defaultdict(list), collections.Counter()
spans, sums, ncopy, copy_ns = [], [], [], []
for c in warm:
    spans.append(c[-1][1] - c[0][0]); sums.append(sum(e[1] - e[0] for e in c))
    prev_end = None
    for e in c:
        dur[e[2]].append(e[1] - e[0])
        if prev_end is not None: gap[e[2]].append(e[0] - prev_end)
        prev_end = max(prev_end or 0, e[1])
    cs = [x for x in copies if c[0][0] <= x[0] <= c[-1][1]]
    ncopy.append(len(cs)); copy_ns.append(sum(x[1] - x[0] for x in cs))
    cnt[tuple(e[2] for e in c)] += 1
us = lambda v: f"{st.mean(v) / 1e3:8.1f}" if v else "       -"
print(f"# {tag}: {len(warm)} warm calls of {len(calls)} (kernel trace {kf.split('/')[-1]})")
print(f"span first start -> last end, us (mean / median): {us(spans)} / {st.median(spans) / 1e3:.1f}")
print(f"sum of kernel durations, us:                      {us(sums)}")
print(f"span - kernel sum, us:                            {st.mean(spans) / 1e3 - st.mean(sums) / 1e3:8.1f}")
print(f"SDMA copies (memory-copy trace) inside the call window: {st.mean(ncopy):.2f} per call (the job table travels as a copy KERNEL, below)")
print("operation             per call   duration us   gap in front us")
for k in dur:
    print(f"{k:22s}{len(dur[k]) / len(warm):8.2f}   {us(dur[k])}      {us(gap[k])}")
print("sequences:", cnt.most_common(3))
