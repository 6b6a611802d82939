#!/usr/bin/env python3
"""Host-side model of the forward's hand-over schedule (adi_fwd_kernel with HO = true, csrc/pde_adi_dev.h): the order in
which a wave polls the counters, stages records by DMA, reads a record's rows and passes its hand-over point, for every set
of round trips issued ahead of their use (PDE_FWD_AHEAD, kAhead* bits).  No GPU, no library: the kernel's spin is unbounded,
so a mistake in the protocol would hang a device, and the order is checked here first.

The model steps 8 waves through a job of 1-3 chunks in arbitrary interleavings (seeded random ones and "one wave runs as
far as it can" ones) and checks
  * liveness: some wave can always move until all are done (every poll is eventually met);
  * a wave only ever waits for the other waves' progress through EARLIER records than the one it is about to use;
  * no ring slot is overwritten while a wave may still read the record in it (a wave may read record r until it has passed
    r's hand-over point);
  * every read of record r finds all eight waves' pieces of r in the slot (a DMA piece lands at any moment between its
    issue and its wave's next hand-over point, a ds_read completes at any moment between its issue and that point).
`mistake` plants a protocol error, to show that the checks see one.

usage: fwd_handover_model.py [seeds]        (prints one line per configuration; exit status 1 on a violation)"""
import random
import sys

WAVES, RING = 8, 4
# kAheadPoll is what the kernel kept; the orders of the candidates that were measured and dropped (rows of the x sweep in
# front of the y sweep's trailing re-layout, the first plane fetched in the prologue, rows in front of the exchange of
# planes) stay in the model: whoever tries them again starts from a checked order
ROWS, POLL, HEAD, CHUNK = 1, 2, 4, 8
MISTAKES = ("stage_before_wait", "trust_short_poll", "wait_for_own_record")


class Violation(Exception):
    pass


def wave_ops(chunks, steps, pair_x, ahead, mistake=None):
    """The protocol events of one wave in program order, as the kernel's chunk loop and sweep() issue them."""
    rpc = 1 + 2 * steps if pair_x else 3 * steps
    ntot = chunks * rpc
    ops, n, rows_in = [], 0, False

    def ask(n):                                  # ho_wait(), ho_stage(), load_fwd_rows()
        if mistake == "stage_before_wait":
            if n + 2 < ntot:
                ops.append(("stage", n + 2))
            ops.append(("wait", n))
        else:
            ops.append(("wait", n))
            if n + 2 < ntot:
                ops.append(("stage", n + 2))
        ops.append(("read", n))

    for _ in range(chunks):
        for s in range(3 * steps):
            axis_y = s % 3 == 1
            staged = not (s % 3 == 0 and pair_x and s != 0)
            if staged and not rows_in:
                ask(n)
            rows_in = False
            if staged:
                if (ahead & POLL) and n >= 1:
                    ops.append(("poll", n - 1))   # ho_poll(): where the solve begins
                ops.append(("pass", n))           # ho_pass(): after the solve
                n += 1
            if axis_y and (ahead & ROWS):         # in front of the y sweep's trailing re-layout
                ask(n)
                rows_in = True
        if (ahead & CHUNK) and n < ntot:          # in front of the exchange of planes
            ask(n)
            rows_in = True
    assert n == ntot
    return ops, ntot


class Model:
    def __init__(self, chunks, steps, pair_x, ahead, mistake=None):
        self.ahead, self.mistake = ahead, mistake
        progs = [wave_ops(chunks, steps, pair_x, ahead, mistake) for _ in range(WAVES)]
        self.ops = [p[0] for p in progs]
        self.ntot = progs[0][1]
        self.pc = [0] * WAVES
        self.passed = [0] * RING                                  # the counters in LDS
        self.done = [0] * WAVES                                   # records wave w has passed
        self.slot = [[None] * WAVES for _ in range(RING)]         # slot[k][w]: the record whose piece of wave w is there
        for r in (0, 1):                                          # the prologue: records 0 and 1, then the barrier
            if r < self.ntot:
                self.slot[r] = [r] * WAVES
        self.dma = [[] for _ in range(WAVES)]                     # pieces in flight: records
        self.rd = [[] for _ in range(WAVES)]                      # reads in flight: records
        self.polled = [None] * WAVES
        self.polls_met_ahead = self.polls = 0

    def want(self, n):
        return WAVES * (((n - 2) >> 2) + 1)

    def land(self, w, r):
        self.slot[r % RING][w] = r

    def complete_read(self, w, r):
        if self.slot[r % RING] != [r] * WAVES:
            raise Violation(f"wave {w} reads record {r} from a slot that holds {self.slot[r % RING]}")

    def enabled(self, w):
        """The moves wave w can make now: 'op' (its next protocol event), ('land', i), ('read', i)."""
        moves = [("land", i) for i in range(len(self.dma[w]))] + [("rd", i) for i in range(len(self.rd[w]))]
        if self.pc[w] < len(self.ops[w]):
            kind, n = self.ops[w][self.pc[w]]
            if kind != "wait" or self.wait_met(w, n, peek=True):
                moves.append(("op", 0))
        return moves

    def wait_met(self, w, n, peek=False):
        if n < 2:
            return True
        src = n if self.mistake == "wait_for_own_record" else n - 2
        want = WAVES * ((src >> 2) + 1)
        if (self.ahead & POLL) and self.polled[w] is not None:
            if self.polled[w][0] == src and (self.polled[w][1] >= want or self.mistake == "trust_short_poll"):
                return True
        return self.passed[src % RING] >= want

    def move(self, w, mv):
        what, i = mv
        if what == "land":
            self.land(w, self.dma[w].pop(i))
            return
        if what == "rd":
            self.complete_read(w, self.rd[w].pop(i))
            return
        kind, n = self.ops[w][self.pc[w]]
        self.pc[w] += 1
        if kind == "wait":
            if n >= 2:
                src = n if self.mistake == "wait_for_own_record" else n - 2
                self.polls += 1
                if self.polled[w] is not None and self.polled[w][0] == src and self.polled[w][1] >= self.want(n):
                    self.polls_met_ahead += 1
            self.polled[w] = None
        elif kind == "poll":
            self.polled[w] = (n, self.passed[n % RING])           # the counter's value now, used a solve later
        elif kind == "stage":
            old = n - RING
            if old >= 0:
                late = [v for v in range(WAVES) if self.done[v] <= old]
                if late:
                    raise Violation(f"wave {w} stages record {n} over record {old}, which waves {late} may still read")
            self.dma[w].append(n)
        elif kind == "read":
            self.rd[w].append(n)
        elif kind == "pass":                                      # s_waitcnt vmcnt(0) lgkmcnt(0), then the counter
            while self.dma[w]:
                self.land(w, self.dma[w].pop(0))
            while self.rd[w]:
                self.complete_read(w, self.rd[w].pop(0))
            self.passed[n % RING] += 1
            self.done[w] = n + 1

    def finished(self):
        return all(self.pc[w] == len(self.ops[w]) and not self.dma[w] and not self.rd[w] for w in range(WAVES))

    def run(self, pick):
        """pick(model, {wave: moves}) -> (wave, move).  Raises Violation; returns the number of moves made."""
        count = 0
        while not self.finished():
            en = {w: m for w in range(WAVES) if (m := self.enabled(w))}
            if not any(("op", 0) in m for m in en.values()) and all(not self.dma[w] and not self.rd[w] for w in range(WAVES)):
                stuck = {w: self.ops[w][self.pc[w]] for w in range(WAVES) if self.pc[w] < len(self.ops[w])}
                raise Violation(f"no wave can move: {stuck}, counters {self.passed}")
            w, mv = pick(self, en)
            self.move(w, mv)
            count += 1
        return count


def random_pick(seed):
    rng = random.Random(seed)

    def pick(model, en):
        w = rng.choice(sorted(en))
        return w, rng.choice(en[w])
    return pick


def greedy_pick(order, lazy):
    """The first wave of `order` that can move runs; lazy: its DMA pieces and reads complete as late as they may."""
    def pick(model, en):
        for w in order:
            if w in en:
                ops = [m for m in en[w] if m[0] == "op"]
                rest = [m for m in en[w] if m[0] != "op"]
                if lazy:
                    return w, (ops[0] if ops else rest[0])
                return w, (rest[0] if rest else ops[0])
        raise AssertionError
    return pick


def schedules(seeds):
    for sd in range(seeds):
        yield f"random {sd}", random_pick(sd)
    for first in range(WAVES):
        order = [first] + [w for w in range(WAVES) if w != first]
        for lazy in (False, True):
            yield f"wave {first} first{', lazy' if lazy else ''}", greedy_pick(order, lazy)
    yield "last wave first, lazy", greedy_pick(list(reversed(range(WAVES))), True)


def check(chunks, steps, pair_x, ahead, seeds=20, mistake=None):
    """Runs every schedule; returns (runs, moves, polls, polls met ahead).  Raises Violation with the schedule's name."""
    runs = moves = polls = met = 0
    for name, pick in schedules(seeds):
        m = Model(chunks, steps, pair_x, ahead, mistake)
        try:
            moves += m.run(pick)
        except Violation as e:
            raise Violation(f"[{name}] {e}") from None
        runs += 1
        polls += m.polls
        met += m.polls_met_ahead
    return runs, moves, polls, met


def waits_only_for_earlier_records(chunks, steps, pair_x, ahead):
    """Static form of the protocol's rule: when a wave waits before using record n it has passed n - 1 already and asks for
    the others' progress through n - 2, never through a record it has not passed itself."""
    ops, _ = wave_ops(chunks, steps, pair_x, ahead)
    passed = 0
    for kind, n in ops:
        if kind == "pass":
            assert n == passed
            passed += 1
        elif kind == "wait" and n >= 2:
            if not (n - 2 < passed and n <= passed):
                return False
        elif kind == "poll":
            if not n < passed + 1:
                return False
    return True


MASKS = (0, POLL)                               # the sets the library is built with (PDE_FWD_AHEAD_LIST)
CANDIDATES = (0, ROWS, POLL, HEAD, CHUNK, ROWS | POLL, ROWS | POLL | CHUNK, ROWS | POLL | HEAD | CHUNK)

if __name__ == "__main__":
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    bad = 0
    for ahead in CANDIDATES:
        for chunks in (1, 2, 3):
            for steps in (2, 3):
                for pair_x in (1, 0):
                    try:
                        ok = waits_only_for_earlier_records(chunks, steps, pair_x, ahead)
                        runs, moves, polls, met = check(chunks, steps, pair_x, ahead, seeds)
                        print(f"ahead {ahead:2d} chunks {chunks} steps {steps} pair_x {pair_x}: {runs} schedules, {moves} moves, "
                              f"{polls} polls, {met} met by the look ahead; waits for earlier records only: {ok}")
                        bad += 0 if ok else 1
                    except Violation as e:
                        print(f"ahead {ahead:2d} chunks {chunks} steps {steps} pair_x {pair_x}: VIOLATION {e}")
                        bad += 1
    sys.exit(1 if bad else 0)
