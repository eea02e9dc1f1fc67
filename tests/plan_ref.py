"""The planned route of emi_plan_route (include/emi355x.h) restated in numpy, operation by operation: the specification the host
function and the kernels of emi_start_guess_dev are held to bit for bit.  Not a port of the C++: the grid quantities are whole-array
expressions (numpy rounds every elementwise operation once and fuses nothing), and the distances are reached the way they are
DEFINED, by sweeps dist[c] <- min(dist[c], min_a fl(dist[a] + w(a -> c))) over all cells at once from +inf until a sweep changes
nothing -- neither Dijkstra's order (the host) nor the in-place order of the kernel.

Also the line and the bend of emi_start_guess_* (mi355x::initial_guess) for a batch."""
import math

import numpy as np

GROWS = (0.25, 0.1, 0.0)
ELLIPSE, DISC, TRACK = 0, 1, 2
NEIGHBOURS = [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if di or dj]       # the order of the predecessor rule


def static_records(recs):
    """(xc, yc, ct, st, asq, bsq) of the records the planner goes round"""
    out = []
    for r in np.asarray(recs, dtype=np.float64).reshape(-1, 8):
        kind = int(r[0])
        if kind == ELLIPSE:
            q = (r[1], r[2], r[3], r[4], r[5], r[6])
        elif kind == DISC:
            q = (r[1], r[2], np.float64(1.0), np.float64(0.0), r[3], r[3])
        else:
            continue
        if q[4] > 0 and q[5] > 0:
            out.append(q)
    return out


def cell_index(v, lo, h, N):
    q = math.floor((v - lo) / h + 0.5)
    return 0 if not q > 0 else (N - 1 if q > N - 1 else int(q))


class Geom:
    def __init__(self, ends, box, clearance, N):
        f = np.float64
        self.x0, self.y0, self.x1, self.y1 = (f(v) for v in ends)
        self.N = N
        self.span = max(abs(self.x1 - self.x0), abs(self.y1 - self.y0))
        self.room = f(clearance) * self.span
        xl, xu, yl, yu = (f(v) for v in box) if box is not None else (f(-np.inf), f(np.inf), f(-np.inf), f(np.inf))
        if not xl > -1e18 or not xu < 1e18:
            xl, xu = min(self.x0, self.x1) - self.span, max(self.x0, self.x1) + self.span
        if not yl > -1e18 or not yu < 1e18:
            yl, yu = min(self.y0, self.y1) - self.span, max(self.y0, self.y1) + self.span
        self.xl, self.yl = xl, yl
        with np.errstate(all="ignore"):
            self.hx, self.hy = (xu - xl) / f(N - 1), (yu - yl) / f(N - 1)
            self.sd = np.sqrt(self.hx * self.hx + self.hy * self.hy)
        self.ok = bool(self.span > 0 and self.hx > 0 and self.hy > 0)
        if self.ok:
            self.start = cell_index(self.x0, xl, self.hx, N) * N + cell_index(self.y0, yl, self.hy, N)
            self.goal = cell_index(self.x1, xl, self.hx, N) * N + cell_index(self.y1, yl, self.hy, N)

    def step(self, di, dj):
        return self.hy if di == 0 else (self.hx if dj == 0 else self.sd)


def grid_fields(g, stat):
    """cellcost [N][N] and blocked [3][N][N]"""
    N = g.N
    ii = np.arange(N, dtype=np.float64)
    x = (g.xl + ii * g.hx)[:, None] * np.ones((1, N))
    y = (g.yl + ii * g.hy)[None, :] * np.ones((N, 1))
    clear = np.full((N, N), 1e300)
    blocked = np.zeros((3, N, N), dtype=bool)
    with np.errstate(all="ignore"):
        for xc, yc, ct, st, asq, bsq in stat:
            rmin = np.sqrt(min(asq, bsq))
            dx, dy = x - xc, y - yc
            ex, ey = ct * dx - st * dy, st * dx + ct * dy
            c = (np.sqrt(ex * ex / asq + ey * ey / bsq) - 1.0) * rmin
            clear = np.where(c < clear, c, clear)
            for l, grow in enumerate(GROWS):
                G = (1.0 + grow) * (1.0 + grow)
                blocked[l] |= ex * ex / (asq * G) + ey * ey / (bsq * G) < 1.0
        lo = 1e-3 * g.span
        cl = np.where(clear > lo, clear, lo)
        cost = 1.0 + ((g.room / cl) * (g.room / cl) if g.room > 0 else 0.0) * np.ones((N, N))
    for l in range(3):
        blocked[l].flat[g.start] = blocked[l].flat[g.goal] = False
    return cost, blocked


def distances(g, cost, blocked):
    """the fixed point, by sweeps over all cells at once"""
    N = g.N
    dist = np.full((N, N), np.inf)
    dist.flat[g.start] = 0.0
    w = {(di, dj): g.step(di, dj) * cost for di, dj in NEIGHBOURS}
    for _ in range(N * N):
        pad = np.full((N + 2, N + 2), np.inf)
        pad[1:-1, 1:-1] = dist
        new = dist
        for di, dj in NEIGHBOURS:
            new = np.minimum(new, pad[1 + di:N + 1 + di, 1 + dj:N + 1 + dj] + w[(di, dj)])
        new = np.where(blocked, dist, new)
        if np.array_equal(new, dist):
            return dist
        dist = new
    return None


def backtrack(g, dist, cost):
    N = g.N
    cells, c = [], g.goal
    while True:
        if len(cells) == N * N:
            return None
        cells.append(c)
        if c == g.start:
            break
        i, j = divmod(c, N)
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if 0 <= a < N and 0 <= b < N and dist[a, b] + g.step(di, dj) * cost[i, j] == dist[i, j]:
                c = a * N + b
                break
        else:
            return None
    return cells[::-1]


class Route:
    """level, cost, cells and the smoothed path with its arc length; resample(tau) gives (xs, ys)"""

    def __init__(self, level, cost=0.0, cells=(), px=None, py=None, arc=None):
        self.level, self.cost, self.cells, self.px, self.py, self.arc = level, cost, list(cells), px, py, arc

    def resample(self, tau):
        tau = np.asarray(tau, dtype=np.float64)
        xs, ys = np.empty(len(tau)), np.empty(len(tau))
        px, py, arc, L = self.px, self.py, self.arc, len(self.px)
        for k, t in enumerate(tau):
            s = 0.5 * (t + 1.0) * arc[-1]
            seg = 0
            while seg + 2 < L and arc[seg + 1] < s:
                seg += 1
            w = (s - arc[seg]) / (arc[seg + 1] - arc[seg]) if arc[seg + 1] > arc[seg] else 0.0
            w = min(1.0, max(0.0, w))
            xs[k] = px[seg] + w * (px[seg + 1] - px[seg])
            ys[k] = py[seg] + w * (py[seg + 1] - py[seg])
        return xs, ys


def plan(recs, ends, box=None, clearance=0.01, grid=0):
    """(Route, None) or, with a route, (Route, (geometry, cellcost, blocked at its level, distances))"""
    N = grid or 161
    g = Geom(ends, box, clearance, N)
    stat = static_records(recs)
    if not g.ok or not stat:
        return Route(-2), None
    cost, blocked = grid_fields(g, stat)
    for level in range(3):
        dist = distances(g, cost, blocked[level])
        if dist is None:
            return Route(-1), None
        if not dist.flat[g.goal] < np.inf:
            continue
        cells = backtrack(g, dist, cost)
        if cells is None or len(cells) < 2:
            return Route(-1), None
        px = [g.xl + np.float64(c // N) * g.hx for c in cells]
        py = [g.yl + np.float64(c % N) * g.hy for c in cells]
        px[0], py[0], px[-1], py[-1] = g.x0, g.y0, g.x1, g.y1
        for _ in range(3):
            for n in range(1, len(px) - 1):
                px[n] = 0.25 * px[n - 1] + 0.5 * px[n] + 0.25 * px[n + 1]
                py[n] = 0.25 * py[n - 1] + 0.5 * py[n] + 0.25 * py[n + 1]
        arc = [np.float64(0.0)]
        for n in range(1, len(px)):
            dx, dy = px[n] - px[n - 1], py[n] - py[n - 1]
            arc.append(arc[-1] + np.sqrt(dx * dx + dy * dy))
        if not arc[-1] > 0:
            return Route(-1), None
        return Route(level, float(dist.flat[g.goal]), cells, px, py, arc), (g, cost, blocked[level], dist)
    return Route(-1), None


def plan_route(recs, ends, tau, box=None, clearance=0.01, grid=0):
    """(xs, ys, level, cost, cells) as etol_amd.plan_route returns them"""
    r = plan(recs, ends, box, clearance, grid)[0]
    if r.level < 0:
        return None, None, r.level, 0.0, np.zeros(0, dtype=np.int32)
    xs, ys = r.resample(tau)
    return xs, ys, r.level, r.cost, np.asarray(r.cells, dtype=np.int32)


def plan_fields(recs, ends, box=None, clearance=0.01, grid=0):
    """(route, geometry, cellcost, blocked at the route's level, distances) of an instance that has a route: what a test needs to
    check a path against the grid it was found on"""
    r, fields = plan(recs, ends, box, clearance, grid)
    assert fields is not None, "no route"
    return (r,) + fields


# ---- the line and the bend of a batch -------------------------------------------------------------------------------------------
def line(xa, xb, tau):
    """X [B][ns][M]: a + (b - a) 0.5 (tau + 1)"""
    xa, xb, tau = (np.asarray(v, dtype=np.float64) for v in (xa, xb, tau))
    return xa[:, :, None] + (xb - xa)[:, :, None] * 0.5 * (tau + 1.0)[None, None, :]


def bend_rows(X, px, py, tau, bend, box=None):
    """rows px, py of X [B][ns][M] (the lines) bent in place; box [B][4] or None.  The sines are libm's (math.sin), which is what the
    library tabulates on the host; numpy's vectorised sine need not round the same way"""
    sine = np.array([math.sin(1.5707963267948966 * (t + 1.0)) for t in tau])
    for b in range(X.shape[0]):
        lx, ly = X[b, px].copy(), X[b, py].copy()
        dx, dy = lx[-1] - lx[0], ly[-1] - ly[0]
        ln = np.sqrt(dx * dx + dy * dy)
        if not ln > 0:
            continue
        x, y = lx - bend * dy / ln * sine, ly + bend * dx / ln * sine
        if box is not None:
            xl, xu, yl, yu = box[b]
            x = np.where(x < xl, xl, x)
            x = np.where(xu < x, xu, x)
            y = np.where(y < yl, yl, y)
            y = np.where(yu < y, yu, y)
        X[b, px], X[b, py] = x, y
    return X
