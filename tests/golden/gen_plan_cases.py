"""Generates tests/golden/plan_cases.json: small record tables for emi_plan_route / emi_start_guess_* with the level each is built
to end at on the default grid of 161 points, and the level tests/plan_ref.py finds on the coarser grids the tests use (a wall can
leak, a gap can close between grid points: on 9 or 17 points the level is whatever the specification gives, recorded here).

    python tests/golden/gen_plan_cases.py

Records are {kind, c0 .. c6} (include/emi355x.h): kind 0 ellipse {xc, yc, cos, sin, a^2, b^2}, 1 disc {xc, yc, r^2}, 2 track."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import plan_ref as PR  # noqa: E402

GRIDS = (9, 17, 33, 161)


def disc(x, y, r):
    return [1.0, x, y, r * r, 0.0, 0.0, 0.0, 0.0]


def track(t, r):
    return [2.0, float(t), r * r, 0.0, 0.0, 0.0, 0.0, 0.0]


def ellipse(x, y, deg, a, b):
    return [0.0, x, y, math.cos(math.radians(deg)), math.sin(math.radians(deg)), a * a, b * b, 0.0]


LINE = [0.0, 0.0, 10.0, 0.0]
ACROSS = [1.0, 5.0, 9.0, 5.0]
SQUARE = [0.0, 10.0, 0.0, 10.0]


def pair(r, extra):
    """two discs of radius r from the lower and the upper edge of the square [0, 10]^2, centred on x = 5: the way from (1, 5) to
    (9, 5) passes between them, through the cell at y = 5, while 2 r (1 + grow) < 10"""
    return [disc(5.0, 0.0, r), disc(5.0, 10.0, r), extra]


CASES = [
    dict(name="one_disc", recs=[disc(5.0, 0.3, 1.0)], ends=LINE, box=None, level=0),
    # a wall of overlapping discs on x = 5 with one gap round y = 4 (the shape of Monte-Carlo scenario 938)
    dict(name="wall_gap", recs=[disc(5.0, float(y), 1.0) for y in range(-11, 12) if y not in (3, 4, 5)], ends=LINE, box=None, level=0),
    dict(name="rotated_ellipse", recs=[ellipse(5.0, 0.0, 30.0, 3.0, 1.0), track(0, 1.0)], ends=LINE, box=None, level=0),
    dict(name="open_everywhere", recs=pair(3.0, track(0, 1.0)), ends=ACROSS, box=SQUARE, level=0),
    dict(name="gap_closed_at_025", recs=pair(4.3, disc(5.0, 0.0, 0.0)), ends=ACROSS, box=SQUARE, level=1),     # 1.1 r < 5 < 1.25 r
    dict(name="gap_open_at_0_only", recs=pair(4.8, track(1, 0.5)), ends=ACROSS, box=SQUARE, level=2),          # r < 5 < 1.1 r
    dict(name="closed_wall", recs=pair(5.2, disc(2.0, 2.0, 0.5)), ends=ACROSS, box=SQUARE, level=-1),
    dict(name="enclosed_goal", recs=[disc(10.0 + 1.8 * math.cos(math.radians(45 * q)), 1.8 * math.sin(math.radians(45 * q)), 1.0) for q in range(8)],
         ends=LINE, box=None, level=-1),
    dict(name="tracks_only", recs=[track(0, 1.0), track(1, 2.0), disc(5.0, 0.0, 0.0)], ends=LINE, box=None, level=-2),
    dict(name="start_in_grown_disc", recs=[disc(1.1, 0.0, 1.0)], ends=LINE, box=None, level=0),                # |start - centre| = 1.1 < 1.25
    dict(name="ties", recs=[disc(5.0, 0.0, 1.0)], ends=LINE, box=None, level=0),                                # everything mirrors in y = 0
]


def main():
    for c in CASES:
        c["clearance"] = 0.01
        c["levels"] = {}
        for grid in GRIDS:
            c["levels"][str(grid)] = PR.plan_route(c["recs"], c["ends"], [-1.0, 1.0], c["box"], c["clearance"], grid)[2]
        assert c["levels"]["161"] == c["level"], (c["name"], c["levels"])
        print(c["name"], c["levels"])
    with open(os.path.join(HERE, "plan_cases.json"), "w") as f:
        json.dump(CASES, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
