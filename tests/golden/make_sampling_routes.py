#!/usr/bin/env python3
"""``sampling_routes.json``: the trace of every case of ``tests/sampling_routes.py``, as the sampling loops of the
tree this runs in produce it.  It was written from the four hand-written loops (``p_sample_loop`` / ``_strided_loop``,
``sample_loop`` / ``_sample_loop_strided``) before they became one driver; run it again only when the behaviour of
the loops is meant to change, and review the diff of the traces.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sampling_routes.py

Needs no device and no library (the engine is a recording stub).
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import sampling_routes as routes                           # noqa: E402


def main():
    traces = {case: routes.run_case(case) for case in routes.CASES}
    path = os.path.join(HERE, "sampling_routes.json")
    with open(path, "w") as fh:
        json.dump(traces, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"  wrote sampling_routes.json: {len(traces)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
