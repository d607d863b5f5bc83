"""Objectives of the BFGS state tests (test_host_scalar_bfgs.py, test_gpu_device_bfgs.py): the families of
test_host_batch_solver.py, restated with the dimension as a parameter.  Each returns f(x) -> (value, grad)."""
import numpy as np


def rosen_like(scale):
    def f(x):
        x = np.asarray(x, dtype=np.float64)
        v = scale * np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2)
        g = np.zeros_like(x)
        g[:-1] += scale * (-400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1]))
        g[1:] += scale * 200.0 * (x[1:] - x[:-1] ** 2)
        return v, g
    return f


def rippled_bowl(seed, n):
    """A smooth bowl plus a deterministic ripple at the 1e-9 level: line searches fail near the optimum."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)); A = A @ A.T + n * np.eye(n)
    b = rng.standard_normal(n)

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        v = 0.5 * x @ A @ x - b @ x + 1e-9 * np.sum(np.sin(1e5 * x))
        g = A @ x - b + 1e-4 * np.cos(1e5 * x)
        return float(v), g
    return f


def bowl_terms(seed, n):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)); A = A @ A.T / n + np.eye(n)
    b = rng.standard_normal(n)
    return A, b


def quartic_bowl(seed, n):
    """0.5 x^T A x - b^T x + sum(x^4) / 4 with A = R R^T / n + I."""
    A, b = bowl_terms(seed, n)
    return lambda x: (float(0.5 * x @ A @ x - b @ x + 0.25 * np.sum(x ** 4)), A @ x - b + x ** 3)


def batch_of(funs):
    B = len(funs)

    def fun_batch(X, mask):
        vg = [(funs[b](X[b]) if mask[b] else (np.nan, np.zeros(X.shape[1]))) for b in range(B)]
        return np.array([v for v, _ in vg]), np.stack([g for _, g in vg])
    return fun_batch
