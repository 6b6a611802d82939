#!/usr/bin/env python3
"""Diagnostic: the timeline of the hand-over forward (adi_fwd_kernel<32, 4, float, Strang, HO>) at the headline shape, from
the s_memtime stamps of a stamped build (tools/variant.sh fstamp -DPDE_STAMP=1): every wave of every workgroup stamps the
top of the kernel and, for its two chunks, plane loads begun / planes in registers / first sweep done / last sweep done /
stores issued, then the last stores drained.  HW_ID / XCC_ID say which workgroups share a CU and LDS_ALLOC which of the two
came second, so the tool prints how long head, exchange and tail are and how far apart the two workgroups of a CU run.
Every wave also sums, over its whole job, the cycles it spends between a hand-over poll's first look and its being met,
between the request of an x sweep's rows and their arrival where nothing stands between the two, and between the prologue's
first record DMA and the first plane fetch: the round trips PDE_FWD_AHEAD issues ahead of their use.
usage: fwd_timeline.py [stagger [tag [ahead]]]      (stagger: PDE_FWD_STAGGER for this run — 0, 1, <naps>,
t<naps>/<share> — default 0; tag: default fstamp; ahead: PDE_FWD_AHEAD for this run, default: the library's)"""
import ctypes as C
import os
import statistics as S
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["PDE_FWD_STAGGER"] = sys.argv[1] if len(sys.argv) > 1 else "0"
tag = sys.argv[2] if len(sys.argv) > 2 else "fstamp"
if len(sys.argv) > 3:
    os.environ["PDE_FWD_AHEAD"] = sys.argv[3]
os.environ.setdefault("PDECNN_LIB", os.path.join(ROOT, "cnn-with-pde_amd", "lib", f"libpdecnn_{tag}.so"))
import torch  # noqa: E402
import cnn_with_pde_amd.functional as F  # noqa: E402
import cnn_with_pde_amd._lib as L  # noqa: E402

B, Cc, N, steps, NW, NS = 512, 64, 32, 10, 8, 24
g = torch.Generator().manual_seed(3)
ab = (2.0 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))).cuda()
bb = (1.8 * (1 + 0.1 * torch.randn(Cc, N, N, generator=g))).cuda()
asl = (0.1 * torch.randn(Cc, N, N, generator=g)).cuda()
bsl = (0.1 * torch.randn(Cc, N, N, generator=g)).cuda()
u = torch.randn(B, Cc, N, N, generator=g).cuda()
sweeps = [s for st in F.adi_schedule(0.001, 1.0, 1.0, steps, "strang") for s in st]
with torch.no_grad():
    for _ in range(6):
        F.adi_diffuse(u, ab, bb, asl, bsl, sweeps, checkpoints=0)
torch.cuda.synchronize()
lib = L.load()
G = 512                                       # workgroups of the launch: C x 8 groups
buf = (C.c_uint64 * (G * NW * NS))()
lib.pde_fwd_stamps.restype = C.c_int
rc = lib.pde_fwd_stamps(buf, G * NW * NS)
assert rc == 0, rc
st = [[[buf[(b * NW + w) * NS + i] for i in range(NS)] for w in range(NW)] for b in range(G)]
assert all(st[b][w][0] for b in range(G) for w in range(NW)), "a workgroup left no stamps: not a stamped hand-over launch"

NAMES = {0: "kernel top", 1: "c0 loads begin", 2: "c0 planes in", 3: "c0 sweep 0 done", 4: "c0 sweeps done", 5: "c0 stores out",
         6: "c1 loads begin", 7: "c1 planes in", 8: "c1 sweep 0 done", 9: "c1 sweeps done", 10: "c1 stores out", 11: "drained"}
med = S.median
# shader clock: s_memtime ticks per 100 MHz tick over the whole wave
mhz = med([(w[11] - w[0]) / max(1, (w[13] - w[12])) * 100.0 for b in st for w in b])
us = lambda cyc: cyc / mhz
print(f"stagger {os.environ['PDE_FWD_STAGGER']}, ahead {os.environ.get('PDE_FWD_AHEAD', 'default')}: shader clock {mhz:.0f} MHz (s_memtime against the 100 MHz counter, median over waves)")


def where(b):
    hid, xcc = st[b][0][14] & 0xffffffff, (st[b][0][14] >> 32) & 0xf
    return (xcc, (hid >> 13) & 7, (hid >> 12) & 1, (hid >> 8) & 0xf)


cus = {}
for b in range(G):
    cus.setdefault(where(b), []).append(b)
base = lambda b: st[b][0][15] & 0xfff
pairs = [sorted(v, key=base) for v in cus.values() if len(v) == 2]
print(f"{len(cus)} CUs; {len(pairs)} hold two workgroups; LDS_BASE differs inside {sum(base(a) != base(b) for a, b in pairs)} pairs; "
      f"values seen: {sorted({base(b) for b in range(G)})}; raw LDS_ALLOC: {sorted({hex(st[b][0][15]) for b in range(G)})}")
print(f"second-dispatched (higher block index) is the one with the higher LDS_BASE in {sum(a < b for a, b in pairs)} pairs of {len(pairs)}")
ph = {b: (1 if base(b) else 0) for b in range(G)}

# the launch as one CU sees it (the s_memtime counters of two CUs are not compared: they differ by milliseconds)
span = [us(max(st[b][w][11] for b in v for w in range(NW)) - min(st[b][w][0] for b in v for w in range(NW))) for v in cus.values()]
print(f"first top to last drained on one CU, us: median {med(span):.1f} [{min(span):.1f} .. {max(span):.1f}]")

SPANS = [("head: c0 loads begin -> planes in", 1, 2), ("c0 sweeps", 2, 4), ("c0 stores issued", 4, 5),
         ("exchange: c0 sweeps done -> c1 planes in", 4, 7), ("c1 loads begin -> planes in", 6, 7), ("c1 sweeps", 7, 9),
         ("tail: c1 sweeps done -> drained", 9, 11), ("whole wave", 0, 11)]
print("durations in us, median [min .. max] over the waves of phase A (first on its CU) | phase B (second)")
for name, i, j in SPANS:
    row = []
    for p in (0, 1):
        d = [us(st[b][w][j] - st[b][w][i]) for b in range(G) if ph[b] == p for w in range(NW)]
        row.append(f"{med(d):6.2f} [{min(d):6.2f} .. {max(d):6.2f}]" if d else "-")
    print(f"  {name:42s} {row[0]}  |  {row[1]}")
print("offset of phase B behind phase A of the same CU, us (median over the waves of each; median [min .. max] over the pairs)")
for i in range(12):
    d = [us(med([st[b][w][i] for w in range(NW)]) - med([st[a][w][i] for w in range(NW)])) for a, b in pairs]
    if d:
        print(f"  {NAMES[i]:18s} {med(d):7.2f} [{min(d):7.2f} .. {max(d):7.2f}]")
# time in which NO wave of a CU is sweeping (both workgroups in loads/stores): the exposed part of the bursts
exposed = []
for a, b in pairs:
    ev = []
    for blk in (a, b):
        for w in range(NW):
            s_ = st[blk][w]
            ev += [(s_[2], 1), (s_[4], -1), (s_[7], 1), (s_[9], -1)]
    ev.sort()
    t_first, t_last = min(st[x][w][0] for x in (a, b) for w in range(NW)), max(st[x][w][11] for x in (a, b) for w in range(NW))
    n, prev, idle = 0, t_first, 0
    for t, dn in ev:
        if n == 0:
            idle += t - prev
        n += dn
        prev = t
    idle += t_last - prev
    exposed.append(us(idle))
if exposed:
    print(f"time with no wave of the CU sweeping, us: median {med(exposed):.2f} [{min(exposed):.2f} .. {max(exposed):.2f}]")
if pairs:
    a, b = pairs[0]
    t0 = min(st[x][w][0] for x in (a, b) for w in range(NW))
    print(f"one CU {where(a)}: blocks {a} (A) and {b} (B); us since the first wave's top; waves 0-7 of A, then of B")
    for i in range(12):
        print(f"  {NAMES[i]:18s} " + " ".join(f"{us(st[a][w][i] - t0):6.1f}" for w in range(NW)) + "  | " +
              " ".join(f"{us(st[b][w][i] - t0):6.1f}" for w in range(NW)))

# the round trips a wave waits out in the open, summed over its job (slots 16-21)
print("waits per wave over its whole job, us, median [min .. max] over the waves of phase A | phase B")
for name, i, j in (("hand-over polls: first look -> met", 16, 19), ("x sweep rows: request -> arrival, bare", 17, 21),
                   ("prologue: record DMA -> first plane fetch", 18, None)):
    row = []
    for p in (0, 1):
        d = [us(st[b][w][i]) for b in range(G) if ph[b] == p for w in range(NW)]
        k = [st[b][w][j] for b in range(G) if ph[b] == p for w in range(NW)] if j is not None else None
        row.append((f"{med(d):6.2f} [{min(d):6.2f} .. {max(d):6.2f}]" + (f" in {med(k):.0f}" if k else "")) if d else "-")
    print(f"  {name:42s} {row[0]}  |  {row[1]}")
slow = [st[b][w][20] for b in range(G) for w in range(NW)]
npoll = [st[b][w][19] for b in range(G) for w in range(NW)]
print(f"polls not met at the first look: {sum(slow)} of {sum(npoll)} ({100.0 * sum(slow) / max(1, sum(npoll)):.1f} %)")
