"""TEST INFRASTRUCTURE.  Mesh families for make_nodes' `shape` hook (adflow_amd/synth.py): the maps the production meshes are made
of and the wavy unit cube is not, each with a severity parameter, and host-side RECOUNTS from a block's own arrays (the pattern of
tests/adversarial.py) so that a test asserts "this mesh is curved / skewed / clustered / collapsed" before it compares.

  annulus    i around a cylinder (sweep degrees), j along the span, k radially from the wall at r0 = 0.5 with the geometric growth
             r = r0 (1 + 40 s), s = expm1(ln(ratio) z) / (ratio - 1), on 1 % waviness
  sheared    the cube's 2 % waviness with x += tan(angle) (z + y / 2): cells `angle` off orthogonal
  clustered  tanh clustering towards BOTH ends of all three directions, f(u) = (1 + tanh(beta (u - 1/2)) / tanh(beta / 2)) / 2,
             0.5 % waviness
  pole       j the radius from an axis along x, k the azimuth (sweep degrees): the whole jMin face collapses onto the axis (every
             sJ there is exactly zero, the first cells are wedges); the halo nodes behind the axis follow the map, which mirrors
             them through the axis
  units      any of them, or the cube, with `lengths` from UNIT_LENGTHS (powers of two: the scaling itself adds no rounding)

Every shape maps the parameter arrays (X, E, Z) to points (..., 3) and carries wall_distance(points, lengths, origin), the
distance to the wall the map puts on k = kMin.

THRESHOLDS holds, per family, what the recount must give at the shapes the tests use; the figures next to them are the recount's
at (12, 8, 6) / (70, 9, 12), with slack.  A family replaced by the cube fails them (test_hostsim_meshes.py asserts that too).

one_ulp_moved / measures: the pieces of the conditioning floor -- the reference run twice, the second time with every node moved by
one ulp; the change of ITS output is the error floor nobody can be held to, measured on the reference alone.
mesh_checks.reference_floor drives it through the checkers, for every (mesh, entry) pair.
"""
import math

import numpy as np

from adflow_amd.synth import face_metrics, cell_volumes

TP = 2.0 * math.pi


def _wavy(X, E, Z, amp):
    """the cube's waviness (make_nodes), as parameters"""
    return (X + amp * np.sin(TP * E) * np.sin(TP * Z),
            E + amp * np.sin(TP * X) * np.sin(TP * Z + 0.3),
            Z + amp * np.sin(TP * X + 0.7) * np.sin(TP * E))


def _stack(x, y, z):
    return np.stack([x, y, z], axis=-1)


class Shape:
    """a map with its wall distance; `name` and `severity` are what DESIGN §5 tabulates"""
    name = "cube"

    def __call__(self, X, E, Z):
        raise NotImplementedError

    def _unscaled(self, pts, lengths, origin):
        return (np.asarray(pts) - np.asarray(origin, float)) / np.asarray(lengths, float)

    def wall_distance(self, pts, lengths, origin):
        """wall = the plane z = 0 of the map (up to its waviness)"""
        return self._unscaled(pts, lengths, origin)[..., 2] * lengths[2]

    def __repr__(self):
        return f"{self.name}({self.severity})"


class Cube(Shape):
    """the default map written as a shape (the `units` family on the cube, and the recount tests' counter-example)"""
    name = "cube"

    def __init__(self, amp=0.02):
        self.amp = self.severity = amp

    def __call__(self, X, E, Z):
        return _stack(*_wavy(X, E, Z, self.amp))


class Annulus(Shape):
    name = "annulus"

    def __init__(self, ratio=1e4, sweep=120.0, r0=0.5, amp=0.01):
        self.ratio, self.sweep, self.r0, self.amp = float(ratio), float(sweep), float(r0), amp
        self.severity = ratio

    def __call__(self, X, E, Z):
        X, E, Z = _wavy(X, E, Z, self.amp)
        th = math.radians(self.sweep) * X
        s = np.sign(Z) * np.expm1(math.log(self.ratio) * np.abs(Z)) / (self.ratio - 1.0)     # halo nodes below the wall mirror the growth
        r = self.r0 * (1.0 + 40.0 * s)
        return _stack(-r * np.cos(th), E, r * np.sin(th))                                      # (theta, span, r) right-handed

    def wall_distance(self, pts, lengths, origin):
        p = self._unscaled(pts, lengths, origin)
        return (np.hypot(p[..., 0], p[..., 2]) - self.r0) * min(lengths[0], lengths[2])


class Sheared(Shape):
    name = "sheared"

    def __init__(self, angle=60.0, amp=0.02):
        self.angle, self.amp = float(angle), amp
        self.severity = angle

    def __call__(self, X, E, Z):
        x, y, z = _wavy(X, E, Z, self.amp)
        return _stack(x + math.tan(math.radians(self.angle)) * (z + 0.5 * y), y, z)


class Clustered(Shape):
    name = "clustered"

    def __init__(self, beta=6.0, amp=0.005):
        self.beta, self.amp = float(beta), amp
        self.severity = beta

    def f(self, u):
        return 0.5 * (1.0 + np.tanh(self.beta * (u - 0.5)) / math.tanh(0.5 * self.beta))

    def __call__(self, X, E, Z):
        return _stack(*_wavy(self.f(X), self.f(E), self.f(Z), self.amp))


class Pole(Shape):
    name = "pole"

    def __init__(self, sweep=90.0, amp=0.02):
        self.sweep, self.amp = float(sweep), amp
        self.severity = sweep

    def __call__(self, X, E, Z):
        # every perturbation carries a factor that is exactly zero at E = 0: the nodes of one i station coincide on the axis
        x = X + self.amp * np.sin(TP * E) * np.sin(TP * Z)
        r = E * (1.0 + self.amp * np.sin(TP * X) * np.sin(TP * Z + 0.3))
        th = math.radians(self.sweep) * (Z + self.amp * np.sin(TP * X + 0.7) * np.sin(TP * E))
        return _stack(x, r * np.cos(th), r * np.sin(th))                                       # (x, r, theta) right-handed


FAMILIES = {"annulus": Annulus, "sheared": Sheared, "clustered": Clustered, "pole": Pole}
UNIT_LENGTHS = ((2.0 ** -20,) * 3, (2.0 ** 10,) * 3, (2.0 ** 7, 1.0, 2.0 ** -7))


def family(name, **kw):
    return (Cube if name == "cube" else FAMILIES[name])(**kw)


# ----------------------------------------------------------------------------------------------------------------------------------
# recounts, from the block's own arrays
# ----------------------------------------------------------------------------------------------------------------------------------
def _mag(v):
    return np.sqrt((v * v).sum(axis=-1))


def recount(blk):
    """aspect: largest ratio of a cell's extents (volume / mean area of the two faces of a direction);
    turning: largest angle between the first and the last edge of an i line over the nodes 1..il, degrees (sweeps below 180);
    min_angle: smallest angle between two of a cell's mean edge directions, degrees (90 - this = deviation from orthogonality);
    zero_faces: (I, J, K) faces of the owned cells with an area of exactly zero;
    vol_ratio: largest / smallest volume of the owned cells."""
    nx, ny, nz = blk.nx, blk.ny, blk.nz
    x, vol = blk["x"], blk["vol"][2:nx + 2, 2:ny + 2, 2:nz + 2]
    aI = _mag(blk["sI"][1:nx + 2, 1:ny + 1, 1:nz + 1])        # faces i = 1..il of the owned cells (sI starts at face 0)
    aJ = _mag(blk["sJ"][1:nx + 1, 1:ny + 2, 1:nz + 1])        # sJ (1:ie, 0:je, 1:ke): first index starts at CELL 1
    aK = _mag(blk["sK"][1:nx + 1, 1:ny + 1, 1:nz + 2])
    h = np.stack([vol / (0.5 * (aI[:-1] + aI[1:])), vol / (0.5 * (aJ[:, :-1] + aJ[:, 1:])), vol / (0.5 * (aK[:, :, :-1] + aK[:, :, 1:]))])
    xo = x[1:nx + 2, 1:ny + 2, 1:nz + 2]
    e = np.diff(xo, axis=0)
    cosang = (e[0] * e[-1]).sum(axis=-1) / np.maximum(_mag(e[0]) * _mag(e[-1]), 1e-300)
    turning = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).max()
    ei = np.diff(xo, axis=0)
    ei = 0.25 * (ei[:, :-1, :-1] + ei[:, 1:, :-1] + ei[:, :-1, 1:] + ei[:, 1:, 1:])
    ej = np.diff(xo, axis=1)
    ej = 0.25 * (ej[:-1, :, :-1] + ej[1:, :, :-1] + ej[:-1, :, 1:] + ej[1:, :, 1:])
    ek = np.diff(xo, axis=2)
    ek = 0.25 * (ek[:-1, :-1] + ek[1:, :-1] + ek[:-1, 1:] + ek[1:, 1:])
    amin = 90.0
    for a, b in ((ei, ej), (ej, ek), (ek, ei)):
        c = np.abs((a * b).sum(axis=-1)) / (_mag(a) * _mag(b))
        amin = min(amin, float(np.degrees(np.arccos(np.clip(c, 0.0, 1.0))).min()))
    return dict(aspect=float((h.max(axis=0) / h.min(axis=0)).max()), turning=float(turning), min_angle=amin,
                zero_faces=(int((aI == 0.0).sum()), int((aJ == 0.0).sum()), int((aK == 0.0).sum())),
                vol_ratio=float(vol.max() / vol.min()), vol_min=float(vol.min()))


# what the recount must give, per family, at every shape the tests use (smallest: (6, 5, 4); figures: the recount's at
# (12, 8, 6) and (70, 9, 12) with the default severities; see DESIGN §5 for the table)
THRESHOLDS = {
    "annulus": lambda n, blk: n["turning"] > 75.0 and n["vol_ratio"] > 1e2 and n["aspect"] > 10.0 and n["zero_faces"] == (0, 0, 0),
    # (turning: a block that spans half a period of the waviness inside a brick shows up to 20 degrees; two of them 39)
    "sheared": lambda n, blk: n["min_angle"] < 35.0 and n["turning"] < 60.0 and n["zero_faces"] == (0, 0, 0),
    "clustered": lambda n, blk: n["vol_ratio"] > 1e2 and n["aspect"] > 5.0 and n["zero_faces"] == (0, 0, 0),
    "pole": lambda n, blk: n["zero_faces"] == (0, blk.nx * blk.nz, 0) and n["vol_min"] > 0.0,
}


def recount_brick(blocks):
    """the recount of blocks joined along i inside one map, as one mesh: turnings and zero-area faces add up, the volume ratio is
    taken over all blocks; returns (recount, stand-in for the block with the brick's nx and nz)"""
    from types import SimpleNamespace
    rs = [recount(b) for b in blocks]
    vmax = max(float(b["vol"][2:b.nx + 2, 2:b.ny + 2, 2:b.nz + 2].max()) for b in blocks)
    vmin = min(r["vol_min"] for r in rs)
    n = dict(aspect=max(r["aspect"] for r in rs), turning=sum(r["turning"] for r in rs), min_angle=min(r["min_angle"] for r in rs),
             zero_faces=tuple(sum(r["zero_faces"][a] for r in rs) for a in range(3)), vol_ratio=vmax / vmin, vol_min=vmin)
    return n, SimpleNamespace(nx=sum(b.nx for b in blocks), ny=blocks[0].ny, nz=blocks[0].nz)


def assert_family(blk, name=None):
    """the recount of `blk` meets its family's thresholds; returns the recount"""
    name = name or blk.shape.name
    n = recount(blk)
    assert np.all(blk["vol"][2:-2, 2:-2, 2:-2] > 0.0)
    assert THRESHOLDS[name](n, blk), (name, n)
    return n


def zero_length_normals(blk, fid):
    """number of faces of the block's face `fid` (1..6), owned cells, whose normal has length exactly zero: the guards for a
    collapsed face are taken on exactly these"""
    nx, ny, nz = blk.nx, blk.ny, blk.nz
    if fid <= 2:
        s = blk["sI"][1 if fid == 1 else blk.il, 1:ny + 1, 1:nz + 1]
    elif fid <= 4:
        s = blk["sJ"][1:nx + 1, 1 if fid == 3 else blk.jl, 1:nz + 1]
    else:
        s = blk["sK"][1:nx + 1, 1:ny + 1, 1 if fid == 5 else blk.kl]
    return int((_mag(s) == 0.0).sum())


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's own conditioning
# ----------------------------------------------------------------------------------------------------------------------------------
def one_ulp_moved(blk, seed=1):
    """a copy of blk with every node coordinate moved by one ulp up or down and the metrics re-formed.  The direction is a
    pseudo-random function of the coordinate's own bits (and the seed): nodes that coincide stay coincident, so a collapsed
    face stays collapsed."""
    b = blk.copy()
    x = b["x"]
    bits = x.view(np.int64) ^ np.int64(0x5DEECE66D * (2 * seed + 1))
    bits = (bits * np.int64(6364136223846793005) + np.int64(1442695040888963407))
    up = ((bits >> 33) & 1).astype(bool)
    xn = np.where(up, np.nextafter(x, np.inf), np.nextafter(x, -np.inf))
    xn = np.where(x == 0.0, 0.0, xn)                      # an exact zero (the axis of `pole`) stays one
    b["x"] = np.asfortranarray(xn)
    sgn = 1.0 if b.rightHanded else -1.0
    b["sI"], b["sJ"], b["sK"] = (np.asfortranarray(sgn * s) for s in face_metrics(b["x"]))
    b["vol"] = cell_volumes(b["x"])
    b["volRef"] = b["vol"].copy(order="F")
    return b


def measures(a, b):
    """the suite's two measures (tests/util.py) of a against b, without touching the session's worst-local record"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    den = np.abs(b).max()
    g = float(np.abs(a - b).max() / den) if den > 0.0 else float(np.abs(a).max())
    d = np.abs(b) + 1e-6 * den
    loc = float((np.abs(a - b) / d).max()) if np.all(d > 0.0) else float(np.abs(a - b).max())
    return g, loc
