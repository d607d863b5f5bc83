"""Parametric motion-field models: a window's unknowns are K <= 12 coefficients of a polynomial field instead of a theta grid
(DESIGN.md section 20).

With the normalised coordinates u = (x - cx) / s, v = (y - cy) / s and the monomials m = [1, u, v, u u, u v, v v], a model is
(K, cx, cy, s, M) with M a (12, K) matrix: q = M c, Theta_x = sum_j q_j m_j, Theta_y = sum_j q_(6 + j) m_j, in px per unit time like
every theta.  ``MotionModel`` builds M for the named models and is the numpy witness of the engine's kernels: ``field`` evaluates the
contract in its exact order (every product rounded, the sums left to right), so it equals ``Engine.motion_field`` bit for bit, and
``project`` is the adjoint M^T mu that ``Engine.loss_grad_motion`` applies to the dense gradient.

The rotation model is the rotational motion field of a calibrated camera (Longuet-Higgins and Prazdny): camera axes X right, Y down,
Z forward along the optical axis, image coordinates x right, y down, u and v the normalised image coordinates ((cx, cy) the
principal point, s the focal length in px), omega = (omega_x, omega_y, omega_z) the camera's angular velocity in rad per unit time.
A static scene's image then moves with
    Theta_x = s (omega_x u v - omega_y (1 + u u) + omega_z v),     Theta_y = s (omega_x (1 + v v) - omega_y u v - omega_z u).
"""
import numpy as np

from . import _lib as L

NQ = L.MOTION_NQ
NM = 6
KINDS = {'translation': 2, 'similarity': 4, 'affine': 6, 'quadratic': 8, 'rotation': 3, 'polynomial2': 12, 'custom': None}


def _builtin_matrix(kind, s):
    M = np.zeros((NQ, KINDS[kind]))
    X, Y = 0, NM                                   # first rows of the two components; row + j: monomial j of [1, u, v, uu, uv, vv]
    if kind == 'polynomial2':
        return np.eye(NQ)
    if kind == 'rotation':
        M[X + 4, 0] = s; M[Y + 0, 0] = s; M[Y + 5, 0] = s          # omega_x: s u v,          s (1 + v v)
        M[X + 0, 1] = -s; M[X + 3, 1] = -s; M[Y + 4, 1] = -s       # omega_y: -s (1 + u u),   -s u v
        M[X + 2, 2] = s; M[Y + 1, 2] = -s                          # omega_z: s v,            -s u
        return M
    M[X + 0, 0] = 1.0; M[Y + 0, 1] = 1.0                           # every other model starts with the translation (c0, c1)
    if kind == 'similarity':                                       # zoom c2, roll c3
        M[X + 1, 2] = 1.0; M[Y + 2, 2] = 1.0
        M[X + 2, 3] = -1.0; M[Y + 1, 3] = 1.0
    elif kind in ('affine', 'quadratic'):
        M[X + 1, 2] = 1.0; M[X + 2, 3] = 1.0; M[Y + 1, 4] = 1.0; M[Y + 2, 5] = 1.0
        if kind == 'quadratic':
            M[X + 3, 6] = 1.0; M[Y + 4, 6] = 1.0
            M[X + 4, 7] = 1.0; M[Y + 5, 7] = 1.0
    return M


class MotionModel:
    """kind: one of KINDS.  sensor_size: (H, W).  centre: (cx, cy) in px, default ((W - 1) / 2, (H - 1) / 2); scale: the normalising
    length in px, default max(H, W) / 2 - a calibrated user passes the principal point and the focal length.  matrix: the (12, K) M
    of kind 'custom' (1 <= K <= 12).  Every refusal is a ValueError and needs no GPU."""

    def __init__(self, kind, sensor_size, centre=None, scale=None, matrix=None):
        if kind not in KINDS:
            raise ValueError(f'motion model kind {kind!r} unknown; one of {sorted(KINDS)}')
        H, W = int(sensor_size[0]), int(sensor_size[1])
        if H < 1 or W < 1:
            raise ValueError(f'sensor_size {sensor_size!r} invalid')
        cx, cy = ((W - 1) / 2.0, (H - 1) / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
        s = max(H, W) / 2.0 if scale is None else float(scale)
        if not (np.isfinite(cx) and np.isfinite(cy)):
            raise ValueError(f'centre ({cx}, {cy}) is not finite')
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError(f'scale {s} is not a positive finite number')
        if (kind == 'custom') != (matrix is not None):
            raise ValueError("matrix goes with kind 'custom', and only with it")
        if kind == 'custom':
            M = np.array(matrix, dtype=np.float64)
            if M.ndim != 2 or M.shape[0] != NQ or not 1 <= M.shape[1] <= L.MOTION_MAX_COEFFS:
                raise ValueError(f'matrix must be ({NQ}, K) with 1 <= K <= {L.MOTION_MAX_COEFFS}, got {M.shape}')
            if not np.isfinite(M).all():
                raise ValueError('matrix holds a NaN or an infinity')
        else:
            M = _builtin_matrix(kind, s)
        self.kind, self.sensor_size, self.cx, self.cy, self.scale = kind, (H, W), cx, cy, s
        self.matrix = np.ascontiguousarray(M)
        self.matrix.setflags(write=False)
        self.n_coeffs = int(M.shape[1])

    def __repr__(self):
        return f'MotionModel({self.kind!r}, {self.sensor_size}, centre=({self.cx}, {self.cy}), scale={self.scale}, K={self.n_coeffs})'

    def as_struct(self):
        """The eincm_motion_model of this model."""
        m = L.MotionModel(self.n_coeffs, self.cx, self.cy, self.scale)
        flat = self.matrix.reshape(-1)
        m.M[:flat.size] = flat.tolist()
        return m

    # -- the contract, in its exact order --------------------------------------------------------------------------------------
    def _coeffs(self, coeffs):
        c = np.asarray(coeffs, dtype=np.float64)
        if c.ndim not in (1, 2) or c.shape[-1] != self.n_coeffs:
            raise ValueError(f'coeffs must be (K,) or (B, K) with K = {self.n_coeffs}, got {c.shape}')
        return c

    def poly(self, coeffs):
        """q = M c, (12,) or (B, 12): a left-to-right sum over k of rounded products."""
        c = self._coeffs(coeffs)
        M = self.matrix
        q = M[:, 0] * c[..., 0:1]
        for k in range(1, self.n_coeffs):
            q = q + M[:, k] * c[..., k:k + 1]
        return q

    def monomials(self):
        """(u, v, uu, uv, vv), each broadcastable to (H, W): the monomials besides 1, every product rounded once."""
        H, W = self.sensor_size
        u = ((np.arange(W, dtype=np.float64) - self.cx) / self.scale)[None, :]
        v = ((np.arange(H, dtype=np.float64) - self.cy) / self.scale)[:, None]
        return u, v, u * u, u * v, v * v

    def field(self, coeffs):
        """Theta (H, W, 2) of coeffs (K,), or (B, H, W, 2) of (B, K): what k_motion_expand writes, bit for bit."""
        c = self._coeffs(coeffs)
        q = self.poly(c).reshape(-1, NQ)
        u, v, uu, uv, vv = self.monomials()
        H, W = self.sensor_size
        out = np.empty((q.shape[0], H, W, 2))
        for b in range(q.shape[0]):
            for a in range(2):
                p = q[b, NM * a:NM * a + NM]
                out[b, :, :, a] = ((((p[0] + p[1] * u) + p[2] * v) + p[3] * uu) + p[4] * uv) + p[5] * vv
        return out[0] if c.ndim == 1 else out

    def moments(self, dense_grad):
        """mu (12,) of a dense gradient (H, W, 2), or (B, 12) of (B, H, W, 2): mu_j = sum_pix m_j dL/dTheta_x, mu_(6 + j) with Theta_y."""
        G = np.asarray(dense_grad, dtype=np.float64)
        H, W = self.sensor_size
        if G.shape[-3:] != (H, W, 2) or G.ndim not in (3, 4):
            raise ValueError(f'dense_grad must be ({H}, {W}, 2) or (B, {H}, {W}, 2), got {G.shape}')
        one = np.ones((1, 1))
        mono = (one,) + self.monomials()
        Gb = G.reshape((-1, H, W, 2))
        mu = np.array([[(m * Gb[b, :, :, a]).sum() for a in range(2) for m in mono] for b in range(Gb.shape[0])])
        return mu[0] if G.ndim == 3 else mu

    def project_moments(self, mu):
        """M^T mu, a left-to-right sum over j of rounded products: (K,) of (12,), (B, K) of (B, 12)."""
        mu = np.asarray(mu, dtype=np.float64)
        M = self.matrix
        g = M[0] * mu[..., 0:1]
        for j in range(1, NQ):
            g = g + M[j] * mu[..., j:j + 1]
        return g

    def project(self, dense_grad):
        """dL/dc = M^T mu of a dense gradient dL/dTheta: the adjoint of ``field``."""
        return self.project_moments(self.moments(dense_grad))

    def monomial_bounds(self):
        """max |m_j| over the sensor, (6,)."""
        H, W = self.sensor_size
        U = max(abs(0.0 - self.cx), abs(float(W - 1) - self.cx)) / self.scale
        V = max(abs(0.0 - self.cy), abs(float(H - 1) - self.cy)) / self.scale
        return np.array([1.0, U, V, U * U, U * V, V * V])

    def abs_bound(self, coeffs):
        """A bound of |field(coeffs)|: per window the larger of sum_j |q_j| max|m_j| over the two components, then the largest
        window.  The engine forms the same number to pick its LDS capacities; Engine.loss_grad_device takes it as theta_abs_max."""
        q = np.abs(self.poly(coeffs)).reshape(-1, 2, NM)
        mm = self.monomial_bounds()
        s = q[:, :, 0] * mm[0]
        for j in range(1, NM):
            s = s + q[:, :, j] * mm[j]
        return float(s.max())


# -- the contrast landscape over coefficients -------------------------------------------------------------------
def coefficient_grid(model, centre, axes, span, n):
    """The (n ** len(axes), K) candidates of a regular grid through ``centre`` (K,): along every one of the 1 to 3 distinct coefficient
    indices ``axes`` the coefficient takes the n values centre[a] + (i - (n - 1) / 2) * (2 * span / (n - 1)), i = 0 .. n - 1; the others
    stay at the centre.  span: the half-range, a positive number or one per axis.  n: odd and >= 3, so the centre is a candidate.
    axes[0] varies fastest: candidate j has i_k = (j // n ** k) % n along axes[k]."""
    K = model.n_coeffs
    c = np.asarray(centre, dtype=np.float64)
    if c.shape != (K,) or not np.isfinite(c).all():
        raise ValueError(f'centre must be ({K},) finite numbers, got {np.shape(centre)}')
    ax = [a for a in np.atleast_1d(np.asarray(axes)).tolist()]
    if not 1 <= len(ax) <= 3 or any(isinstance(a, bool) or not isinstance(a, int) or not 0 <= a < K for a in ax) or len(set(ax)) != len(ax):
        raise ValueError(f'axes must hold 1 to 3 distinct coefficient indices within 0 .. {K - 1}, got {axes!r}')
    sp = np.asarray(span, dtype=np.float64)
    if sp.shape not in ((), (len(ax),)) or not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError(f'span must be a positive finite number or one per axis, got {span!r}')
    sp = np.broadcast_to(sp, (len(ax),))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 3 or n % 2 == 0:
        raise ValueError(f'n must be an odd integer >= 3, got {n!r}')
    n = int(n)
    out = np.tile(c, (n ** len(ax), 1))
    j = np.arange(n ** len(ax))
    for k, a in enumerate(ax):
        i = (j // n ** k) % n
        out[:, a] = c[a] + (i - (n - 1) / 2) * (2 * sp[k] / (n - 1))
    return out


def landscape_variance(sumsq, n_in, n_cells):
    """The variance of the image of cell counts, sumsq / P - (n_in / P) ** 2 with P = n_cells, in float64: for display.  The search
    itself ranks by the integer ``sumsq``."""
    P = float(n_cells)
    return np.asarray(sumsq, dtype=np.float64) / P - (np.asarray(n_in, dtype=np.float64) / P) ** 2


def warped_pixels(model, coeffs, xs, ys, ts, t_ref):
    """Where the contrast landscape counts one window's events under coeffs (K,): (r_x, r_y, inside) with r = rint(x - Theta * dt) as
    float64, Theta = field(coeffs) at the event's own pixel, dt = ts - t_ref, the product rounded before the subtraction; inside is the
    in-sensor test 0 <= r_x < W and 0 <= r_y < H on the floats (false for a NaN).  The host half of segmentation.seed_motions."""
    H, W = model.sensor_size
    x, y = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64)
    with np.errstate(over='ignore', invalid='ignore'):
        th = model.field(coeffs)[y, x]
        dt = np.asarray(ts, dtype=np.float64) - float(t_ref)
        rx = np.rint(x.astype(np.float64) - th[:, 0] * dt)
        ry = np.rint(y.astype(np.float64) - th[:, 1] * dt)
        inside = (rx >= 0.0) & (rx < float(W)) & (ry >= 0.0) & (ry < float(H))
    return rx, ry, inside
