#!/usr/bin/env python3
"""Diagnostic: launch times (HIP events inside the library) of the headline forward + backward under a list of
PDE_FWD_AHEAD values (bit mask; 2 = hand-over counters polled a solve ahead, 0 = none; a build with more candidates in
PDE_FWD_AHEAD_LIST takes their masks), the method of tools/perf_fwd_stagger.py: 20 calls after 5, one child process per
value and round, the values alternating round by round.  The value "parent" runs the library PDECNN_PARENT_LIB names.
usage: perf_fwd_ahead.py [rounds] [value ...]"""
import os
import subprocess
import sys

from perf_fwd_stagger import child

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
        sys.exit(0)
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    values = sys.argv[2:] or ["0", "2"]
    for r in range(rounds):
        for v in values:
            env = dict(os.environ, PDE_FWD_AHEAD=v)
            if v == "parent":                      # the parent commit's library, given as PDECNN_PARENT_LIB
                env.pop("PDE_FWD_AHEAD")
                env["PDECNN_LIB"] = os.environ["PDECNN_PARENT_LIB"]
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(f"ahead {v}: FAILED ({p.returncode}) {p.stderr[-300:]}", flush=True)
                sys.exit(1)                  # nothing more is started on the device after a failure
            print(f"round {r} ahead {v:>6s}: {p.stdout.strip().splitlines()[-1]}", flush=True)
