#!/usr/bin/env python3
"""Record which kernels the stepper family's calls launch: runs tests/step_route_cases.py's case list (count, findall,
sub on a fresh handle each) and writes mrx_last_kernel_name() after every call.

usage: python tools/record_step_routes.py [out.json [commit]]     (default: tests/golden/step_routes.json, git's HEAD)

The file pins the routes of the commit it was recorded at; tests/test_gpu_step_routes.py holds later commits to it.
Record it again only when a route is changed on purpose, and say so."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import mojo_regex_amd as M  # noqa: E402
import step_route_cases as S  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_routes.json")
    batches = {}
    routes = {}
    for case in S.CASES:
        key = (case.family, case.shape, case.alphabet)
        if key not in batches:
            texts = S.texts_for(case.family, case.shape, case.alphabet)
            batches[key] = (S.make_batch(M, torch, case.shape, texts), sum(len(t) for t in texts))
        names, _ = S.run_case(M, torch, case, *batches[key])
        routes[case.id] = names
        print("%-60s %s" % (case.id, " ".join(names)), flush=True)
    if len(sys.argv) > 2:
        commit = sys.argv[2]
    else:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    with open(out, "w") as f:
        json.dump({"recorded_at": commit, "routes": routes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(routes)))


if __name__ == "__main__":
    main()
