#!/usr/bin/env python3
"""Times of one rung change's worth of track centres by the two routes: the device call on waypoint tables the context keeps
(emi_tracks_from_waypoints_dev) and the existing route through the host (emi_track_centres per track, then emi_set_tracks, which
uploads [sets][tracks][M] doubles twice).  Nothing is gated; JSON lines go to profiles/track_times.jsonl.

  python tools/track_times.py [--shapes 64x4x257,128x4x1024] [--calls 100] [--rounds 3] [--waypoints 16]

Shapes are sets x tracks x nodes; every track has `waypoints` waypoints over [t0, tf].  Device call: the median of `calls` single calls
by HIP events on the context's stream (emi_timer_*), identity map.  Host route: the median of `calls` wall times of the Python loop
over emi_track_centres plus emi_set_tracks (which synchronises).  The two alternate over `rounds` rounds.  The centres of the two
routes are compared bit for bit once, before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import etol_amd as E

T0, TF = 0.0, 4.0


def run_shape(sets, tracks, M, calls, rounds, nway):
    rng = np.random.default_rng(sets * 1000 + M)
    t = np.sort(rng.uniform(T0, TF, (sets, tracks, nway)), axis=2)
    t[:, :, 0], t[:, :, -1] = T0, TF
    assert (np.diff(t, axis=2) > 0).all()
    x, y = rng.uniform(0, 10, t.shape), rng.uniform(0, 10, t.shape)
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_track_waypoints(t, x, y)
    xc, yc = np.empty((sets, tracks, M)), np.empty((sets, tracks, M))

    def host_route():
        for s in range(sets):
            for k in range(tracks):
                xc[s, k], yc[s, k] = E.track_centres(t[s, k], x[s, k], y[s, k], ev.node_t)
        ev.set_tracks(xc, yc)

    def time_device():
        ms = []
        for _ in range(calls):
            ev.timer_start()
            ev.tracks_from_waypoints()
            ms.append(ev.timer_stop())
        return statistics.median(ms)

    def time_host():
        ms = []
        for _ in range(calls):
            a = time.perf_counter()
            host_route()
            ms.append(1e3 * (time.perf_counter() - a))
        return statistics.median(ms)

    host_route()
    want = ev.get_tracks()
    ev.tracks_from_waypoints()
    got = ev.get_tracks()
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
    for _ in range(5):                      # warm-up of both
        ev.tracks_from_waypoints()
        host_route()
    ev.synchronize()
    dev, host = [], []
    for _ in range(rounds):
        dev.append(time_device())
        host.append(time_host())
    ev.close()
    return dict(what="track centres of one rung change", sets=sets, tracks=tracks, M=M, waypoints=nway, calls=calls, rounds=rounds,
                ms_device=dev, ms_host_route=host, ms_device_median=statistics.median(dev), ms_host_route_median=statistics.median(host),
                ratio=statistics.median(host) / statistics.median(dev), bytes_uploaded_by_the_host_route=2 * sets * tracks * M * 8,
                same_bits=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x4x257,128x4x1024")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_times.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for s in a.shapes.split(","):
            r = run_shape(*(int(v) for v in s.split("x")), a.calls, a.rounds, a.waypoints)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
