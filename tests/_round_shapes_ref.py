"""numpy float32 restatement of the round and concave shape rules (include/planeverb_amd.h, "Round and concave shapes"): disc,
capsule, wall path and the even-odd simple polygon, on the cell centres of the convex rule.  Every operation is float32 in the
order the header's brackets give, so the restatement is exact."""
import numpy as np

from _shapes_ref import coverage as convex_coverage

F = np.float32
DISC, CAPSULE, WALL_PATH, POLYGON, CONVEX = 1, 2, 3, 4, 0


def centres(gx, gy, dx):
    dx = F(dx)
    X = ((np.arange(gx, dtype=np.float32) + F(0.5)) * dx)[:, None]
    Y = ((np.arange(gy, dtype=np.float32) + F(0.5)) * dx)[None, :]
    return X, Y


def _grid(ok, gx, gy):
    out = np.zeros((gx + 1, gy + 1), np.uint8)
    out[:gx, :gy] = ok
    return out


def disc_coverage(c, r, gx, gy, dx):
    c, r = np.asarray(c, np.float32).reshape(2), F(r)
    X, Y = centres(gx, gy, dx)
    with np.errstate(all="ignore"):
        ddx, ddy = X - c[0], Y - c[1]
        return _grid((ddx * ddx) + (ddy * ddy) <= r * r, gx, gy)


def _capsule(a, b, r, X, Y):
    with np.errstate(all="ignore"):
        ex, ey = b[0] - a[0], b[1] - a[1]
        wx, wy = X - a[0], Y - a[1]
        ee = (ex * ex) + (ey * ey)
        if ee == 0:
            t = np.zeros(np.broadcast(wx, wy).shape, np.float32)
        else:
            t = ((wx * ex) + (wy * ey)) / ee
            t = np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(np.float32)
        qx, qy = wx - (t * ex), wy - (t * ey)
        return (qx * qx) + (qy * qy) <= r * r


def capsule_coverage(a, b, r, gx, gy, dx):
    X, Y = centres(gx, gy, dx)
    return _grid(_capsule(np.asarray(a, np.float32), np.asarray(b, np.float32), F(r), X, Y), gx, gy)


def wall_path_coverage(xy, r, gx, gy, dx):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    X, Y = centres(gx, gy, dx)
    ok = np.zeros((gx, gy), bool)
    for i in range(len(xy) - 1):
        ok |= _capsule(xy[i], xy[i + 1], F(r), X, Y)
    return _grid(ok, gx, gy)


def polygon_coverage(xy, gx, gy, dx):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    X, Y = centres(gx, gy, dx)
    inside = np.zeros((gx, gy), bool)
    n = len(xy)
    with np.errstate(all="ignore"):
        for i in range(n):
            a, b = xy[i], xy[(i + 1) % n]
            straddle = (a[1] > Y) != (b[1] > Y)
            xi = (((b[0] - a[0]) * (Y - a[1])) / (b[1] - a[1])) + a[0]
            inside ^= straddle & (X < xi)
    return _grid(inside, gx, gy)


def coverage(shape, gx, gy, dx):
    """shape = (kind, points, radius): uint8 (gx+1) x (gy+1)"""
    kind, pts, r = shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if kind == DISC:
        return disc_coverage(pts[0], r, gx, gy, dx)
    if kind == CAPSULE:
        return capsule_coverage(pts[0], pts[1], r, gx, gy, dx)
    if kind == WALL_PATH:
        return wall_path_coverage(pts, r, gx, gy, dx)
    if kind == POLYGON:
        return polygon_coverage(pts, gx, gy, dx)
    return convex_coverage(pts, gx, gy, dx)


def compose(beta, R, shapes, gx, gy, dx):
    """beta / R of the AABB layer and the live shapes [((kind, points, radius), absorption)], oldest first"""
    b, r = beta.copy(), R.copy()
    for shape, a in shapes:
        c = coverage(shape, gx, gy, dx).astype(bool)
        b[c] = 0
        r[c] = F(a)
    return b, r


def random_simple_polygon(rng, cx, cy, radius, n):
    """a star-shaped (so simple), usually concave polygon: one vertex per angular slot (every gap below pi, so the centre sees
    every edge), radii that swing between 35 % and 100 %"""
    ang = 2 * np.pi * (np.arange(n) + 0.4 * rng.uniform(0, 1, n)) / n + rng.uniform(0, 2 * np.pi)
    rad = radius * rng.uniform(0.35, 1.0, n)
    xy = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).astype(np.float32)
    return xy if rng.random() < 0.5 else xy[::-1].copy()


def random_path(rng, size, n, step):
    p = [rng.uniform(0.0, size, 2)]
    for _ in range(n - 1):
        p.append(p[-1] + rng.uniform(-step, step, 2))
    return np.asarray(p, np.float32)
