"""One battery of tests/process_knob_cases.py in a process of its own, under whatever STMMQR_* environment it was started with (the
PROCESS rows of csrc/stmmqr_knobs.h are fixed at their first use: only a fresh process sees another value).

    python tests/process_knob_child.py BATTERY OUT.json          BATTERY: rider | parts | batch

Writes {"battery", "digests": {case: sha256}, "reports": {case: [[host, unfr, uncb, umaxsl, rspw, uy], ...]}, "seconds": {case: s},
"wall": s} to OUT.json.  Every rider case is also factorized with options.lookahead = 0 in this process and must give the same bits,
and every factorization is compared with the CPU oracle; a failed assertion ends the process with exit code 1 and the message on
stderr."""
import importlib
import json
import sys
import time
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def run(battery):
    import process_knob_cases as pk
    from stmmqr_testlib import Oracle
    pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert pkg.device_count() >= 1, "no GPU"
    out = {"battery": battery, "digests": {}, "reports": {}, "seconds": {}}
    if battery == "rider":
        oracle = Oracle()
        for case in pk.RIDER_CASES:
            t0 = time.monotonic()
            out["digests"][case.name], out["reports"][case.name] = pk.run_rider_case(pkg, oracle, case)
            out["seconds"][case.name] = round(time.monotonic() - t0, 3)
    elif battery == "parts":
        out["digests"] = pk.run_parts_battery(pkg, Oracle())
    elif battery == "batch":
        out["digests"] = pk.run_batch_battery(pkg)
    else:
        raise SystemExit(f"unknown battery {battery!r}: rider, parts or batch")
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    t0 = time.monotonic()
    try:
        out = run(argv[1])
    except AssertionError:
        traceback.print_exc()
        return 1
    out["wall"] = round(time.monotonic() - t0, 3)
    Path(argv[2]).write_text(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
