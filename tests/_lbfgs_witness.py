"""Witness of the limited-memory direction (test_host_lbfgs.py, test_gpu_lbfgs.py): the classical two-loop recursion on the vectors
themselves, in np.longdouble, and the random histories the direction tests run on.  Nothing here shares code with batch_solver."""
import numpy as np

LD = np.longdouble


def two_loop(S, Y, g, initial_scale):
    """-H g for the pairs S[i], Y[i] (oldest first): q = g; a_i = (s_i . q) / (s_i . y_i), q -= a_i y_i, newest to oldest; r = gamma q
    with gamma = s.y / y.y of the newest pair ('last_pair') or 1 ('identity', or no pair); r += s_i (a_i - (y_i . r) / (s_i . y_i)),
    oldest to newest.  Every operation in long double; the result is returned in long double."""
    S, Y = [np.asarray(s, dtype=LD) for s in S], [np.asarray(y, dtype=LD) for y in Y]
    q = np.asarray(g, dtype=LD).copy()
    a = [None] * len(S)
    for i in reversed(range(len(S))):
        a[i] = (S[i] @ q) / (S[i] @ Y[i])
        q = q - a[i] * Y[i]
    gamma = (S[-1] @ Y[-1]) / (Y[-1] @ Y[-1]) if (S and initial_scale == 'last_pair') else LD(1)
    r = gamma * q
    for i in range(len(S)):
        beta = (Y[i] @ r) / (S[i] @ Y[i])
        r = r + S[i] * (a[i] - beta)
    return -r


def random_spd(rng, n):
    """Q diag(d) Q^T with d in [0.5, 2]: y = A s has y . s >= 0.5 s . s"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (q * rng.uniform(0.5, 2.0, n)) @ q.T


def ordered_pairs(w):
    """The pairs of a host window (batch_solver._LimitedWindow) oldest first."""
    slots = [(w.head + i) % w.m for i in range(w.count)]
    return [w.S[k] for k in slots], [w.Y[k] for k in slots]
