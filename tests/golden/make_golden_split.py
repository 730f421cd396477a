#!/usr/bin/env python3
"""Generate tests/golden/split_ratio.json by running the REFERENCE's MultitaskData.cal_split (model/dataset/dataloader.py:428-480) on CPU
over recorded lane sets.

dataloader.py imports cv2 and imgaug at module level, so the function is taken out of the file with `ast` and executed on its own, with
`np.RankWarning` bound to numpy 2's np.exceptions.RankWarning (its numpy-1 meaning: a rank-deficient fit returns (False, None)).
Each case: {"name", "width", "height", "lanes" ({"Lines": [[{"x", "y"}, ...]]}, as dataset.parse_own_label returns), "ok", "ratio"}.
Run:  python tests/golden/make_golden_split.py"""
import ast
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/model/dataset/dataloader.py"
sys.dont_write_bytecode = True


class _NumpyOne:
    """numpy with the numpy-1 name the reference catches"""
    RankWarning = np.exceptions.RankWarning

    def __getattr__(self, name):
        return getattr(np, name)


def _reference_cal_split():
    tree = ast.parse(open(REF).read())
    fn = next(n for c in tree.body if isinstance(c, ast.ClassDef) for n in c.body
              if isinstance(n, ast.FunctionDef) and n.name == "cal_split")
    fn.decorator_list = []
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    env = {"np": _NumpyOne(), "warnings": warnings}
    exec(compile(mod, REF, "exec"), env)
    return env["cal_split"]


class _Image:
    def __init__(self, h, w):
        self.shape = (h, w, 3)


def _line(pts, as_str=False):
    f = (lambda v: repr(float(v))) if as_str else float
    return [{"x": f(x), "y": f(y)} for x, y in pts]


def _cases():
    W, H = 1280, 720
    c = [
        ("no_lanes", W, H, []),
        ("one_lane_positive", W, H, [_line([(100, 700), (400, 400)])]),
        ("one_lane_negative", W, H, [_line([(900, 700), (700, 400)])]),
        ("all_positive", W, H, [_line([(100, 700), (400, 400)]), _line([(300, 710), (500, 420), (600, 300)])]),
        ("all_negative", W, H, [_line([(1100, 700), (800, 400)]), _line([(900, 715), (700, 380)])]),
        ("mixed_two", W, H, [_line([(200, 700), (550, 380)]), _line([(1100, 700), (720, 380)])]),
        ("mixed_four", W, H, [_line([(50, 690), (300, 500), (560, 360)]), _line([(400, 719), (600, 380)]),
                              _line([(900, 719), (700, 380)]), _line([(1250, 640), (1000, 500), (760, 360)])]),
        # a lane on the bottom edge (flipped y 0) fits a slope of exactly 0; a horizontal lane elsewhere fits a slope of about 1e-16
        ("slope_zero", W, H, [_line([(200, 700), (550, 380)]), _line([(100, H), (600, H), (900, H)]),
                              _line([(1100, 700), (720, 380)])]),
        ("slope_zero_only", W, H, [_line([(100, H), (600, H)])]),
        ("horizontal_not_exact", W, H, [_line([(200, 700), (550, 380)]), _line([(100, 500), (600, 500)])]),
        ("vertical", W, H, [_line([(200, 700), (550, 380)]), _line([(640, 700), (640, 500), (640, 380)])]),
        ("one_point", W, H, [_line([(200, 700), (550, 380)]), _line([(900, 600)])]),
        ("empty_lane", W, H, [_line([(200, 700), (550, 380)]), []]),
        ("two_point", W, H, [_line([(200, 700), (550, 380)]), _line([(1000, 650), (760, 390)])]),
        ("y_out_of_order", W, H, [_line([(450, 450), (200, 700), (550, 380), (300, 600)]),
                                  _line([(800, 420), (1100, 700), (720, 380), (950, 560)])]),
        ("fractional_truncated", W, H, [_line([(199.9, 700.7), (550.2, 380.99)]), _line([(1100.6, 699.5), (-0.5, 380.2)])]),
        ("string_coords", W, H, [_line([(210.5, 705.25), (560, 370)], True), _line([(1090, 690.75), (730.5, 375)], True)]),
        ("x_outside_left", W, H, [_line([(-400, 719), (500, 380)]), _line([(-100, 719), (-300, 380)])]),
        ("x_outside_right", W, H, [_line([(1500, 719), (1900, 380)]), _line([(1700, 719), (1300, 380)])]),
        ("y_ties", W, H, [_line([(300, 700), (250, 700), (500, 400), (480, 400)]), _line([(1000, 700), (1040, 700), (800, 400)])]),
        ("fullhd_mixed", 1920, 1080, [_line([(300, 1070), (700, 800), (900, 620)]), _line([(1700, 1060), (1200, 760), (1000, 620)])]),
    ]
    g = np.random.default_rng(20261016)
    for i in range(12):
        w, h = ((1280, 720), (1920, 1080), (2560, 1440))[i % 3]
        lanes = []
        for _ in range(int(g.integers(2, 5))):
            n = int(g.integers(2, 12))
            x0, x1 = g.uniform(-0.2 * w, 1.2 * w), g.uniform(0.3 * w, 0.7 * w)
            y0, y1 = g.uniform(0.8 * h, h), g.uniform(0.35 * h, 0.6 * h)
            t = np.sort(g.uniform(0, 1, n))
            pts = [(round(float(x0 + (x1 - x0) * s + g.normal(0, 3)), 2), round(float(y0 + (y1 - y0) * s), 2)) for s in t]
            if g.integers(2):
                pts = pts[::-1]
            lanes.append(_line(pts, bool(g.integers(2))))
        c.append(("random_%02d" % i, w, h, lanes))
    return c


def main():
    cal_split = _reference_cal_split()
    out = []
    for name, w, h, lines in _cases():
        lanes = {"Lines": lines}
        ok, ratio = cal_split(_Image(h, w), lanes)
        out.append({"name": name, "width": w, "height": h, "lanes": lanes, "ok": bool(ok), "ratio": None if ratio is None else float(ratio)})
    by = {c["name"]: c for c in out}
    assert not any(by[k]["ok"] for k in ("no_lanes", "slope_zero", "slope_zero_only", "vertical", "one_point", "empty_lane"))
    assert by["horizontal_not_exact"]["ok"] and by["mixed_two"]["ok"]
    assert sum(c["ok"] for c in out) >= 10 and sum(not c["ok"] for c in out) >= 10
    path = os.path.join(HERE, "split_ratio.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote %s: %d cases, %d with a split" % (path, len(out), sum(c["ok"] for c in out)))


if __name__ == "__main__":
    main()
