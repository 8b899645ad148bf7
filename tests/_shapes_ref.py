"""numpy float32 restatement of the shape model (include/planeverb_amd.h, "Shapes"): oriented-box vertices, the cell-centre
coverage rule and the composition over the AABB layer.  Every operation is float32, so the restatement is exact."""
import numpy as np

F = np.float32


def obb_vertices(px, py, w, h, ax, ay):
    px, py, w, h, ax, ay = (F(v) for v in (px, py, w, h, ax, ay))
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(ax * ax + ay * ay)
        ux, uy = ax * inv, ay * inv
        vx, vy = -uy, ux
        hw, hh = w / F(2), h / F(2)
        wx, wy, hx, hy = hw * ux, hw * uy, hh * vx, hh * vy
        return np.array([[(px - wx) - hx, (py - wy) - hy], [(px + wx) - hx, (py + wy) - hy],
                         [(px + wx) + hx, (py + wy) + hy], [(px - wx) + hx, (py - wy) + hy]], np.float32)


def ccw(xy):
    """the vertex list counter-clockwise (shoelace sign in float64)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    area = np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)
    return xy if area > 0 else xy[::-1].copy()


def coverage(xy, gx, gy, dx):
    """uint8 (gx+1) x (gy+1): cells whose centre passes every edge test; the ghost row and column stay 0"""
    xy = ccw(xy)
    dx = F(dx)
    X = ((np.arange(gx, dtype=np.float32) + F(0.5)) * dx)[:, None]
    Y = ((np.arange(gy, dtype=np.float32) + F(0.5)) * dx)[None, :]
    ok = np.ones((gx, gy), bool)
    n = len(xy)
    with np.errstate(all="ignore"):
        for i in range(n):
            a, b = xy[i], xy[(i + 1) % n]
            ex, ey = b[0] - a[0], b[1] - a[1]
            ok &= ((ex * (Y - a[1])) - (ey * (X - a[0]))) >= F(0)
    out = np.zeros((gx + 1, gy + 1), np.uint8)
    out[:gx, :gy] = ok
    return out


def compose(beta, R, shapes, gx, gy, dx):
    """beta / R of the AABB layer and the live shapes [(vertices, absorption)] in sequence order (oldest first)"""
    b, r = beta.copy(), R.copy()
    for xy, a in shapes:
        c = coverage(xy, gx, gy, dx).astype(bool)
        b[c] = 0
        r[c] = F(a)
    return b, r


def random_convex(rng, cx, cy, radius, n):
    """a convex polygon of n vertices on a jittered circle, counter-clockwise"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = radius * rng.uniform(0.6, 1.0)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).astype(np.float32)
