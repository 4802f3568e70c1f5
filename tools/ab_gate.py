"""Gate of a same-process A/B (tools/ab_step.py ON1 OFF1 ON2 OFF2): reads the
JSON line of the log and reports

    spread = max(|median(ON1) - median(ON2)|, |median(OFF1) - median(OFF2)|)
    gain   = mean of the OFF medians - mean of the ON medians

The gain counts when it is at least 3 x spread and at least 1 % of the OFF
median (twice the +-0.5 % in-process spread of DESIGN.md §14).

    python3 tools/ab_gate.py LOG base twolaunchbnbwd

(tools/ab_step.py --gate ON OFF prints the same line after its own.)
"""
import json
import sys


def gate(res, on, off):
    m = {k: v["ms_median"] for k, v in res.items()}
    on1, on2, off1, off2 = m[on + "1"], m[on + "2"], m[off + "1"], m[off + "2"]
    spread = max(abs(on1 - on2), abs(off1 - off2))
    off_med = (off1 + off2) / 2
    gain = off_med - (on1 + on2) / 2
    ok = gain >= 3 * spread and gain >= 0.01 * off_med
    return {"on_ms": [on1, on2], "off_ms": [off1, off2], "spread_ms": round(spread, 4),
            "gain_ms": round(gain, 4), "gain_pct": round(100 * gain / off_med, 2),
            "gate": bool(ok)}


def main():
    log, on, off = sys.argv[1:4]
    res = None
    for line in open(log):
        if line.startswith("{") and '"gate"' not in line:  # ab_step's line, not a gate line
            res = json.loads(line)
    if res is None:
        sys.exit("no JSON line in " + log)
    print(json.dumps(gate(res, on, off)))


if __name__ == "__main__":
    main()
