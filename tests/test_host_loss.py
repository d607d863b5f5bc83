"""The loss's scalar assembly (csrc/eincm_loss.h: the functions k_final and the host's assemblies share) on the CPU.

tests/host/loss_check.cpp is built once per session with the address and undefined-behaviour sanitizers (tests/_host_check.py) and
-ffp-contract=off, and run once, as a child process, over every case of this module; nothing is preloaded.  Three kinds of check:
  * pinned to the reference: the per-image values its 14 loss fixtures recorded (tests/golden/ref_*.npz with `params` and `obj_*`)
    through image_terms + assemble_window give the recorded value and means to 1e-12 relative (tests/test_reference_golden.py's bar);
  * a witness: every function restated below in plain Python floats with the same operation order, compared bit for bit;
  * loss_weights is the derivative of the forward terms: a perturbation of 2^-20 of one image's term moves the value by the weight
    times the perturbation, to 1e-9 relative (the formula is linear in each term: only rounding separates the two).
"""
import glob
import math
import os
import sys

import numpy as np
import pytest

import _host_check as HC

EPS = sys.float_info.epsilon
NAN = float('nan')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
IG_WAVES = 4                            # k_imgrad strips per workgroup (IG_NT / 64)


@pytest.fixture(scope='session')
def loss_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'loss_check', extra=['-ffp-contract=off'])


CASES = {}


def _case(name, *tokens):
    return HC.add_case(CASES, name, *tokens)


@pytest.fixture(scope='module')
def out(loss_check, tmp_path_factory):
    return HC.run(loss_check, CASES, tmp_path_factory, 'loss_cases')


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)]) \
        and np.array_equal(np.isnan(got), np.isnan(want))


# ================================================================================================
# the witness: plain Python floats, the operation order of eincm_loss.h
# ================================================================================================
class EP:
    def __init__(self, alpha, beta, gamma, delta, lvl, kind, want_div, want_tv):
        self.alpha, self.beta, self.gamma, self.delta = float(alpha), float(beta), float(gamma), float(delta)
        self.lvl, self.kind, self.want_div, self.want_tv = int(lvl), int(kind), int(want_div), int(want_tv)

    def tokens(self):
        return (self.alpha, self.beta, self.gamma, self.delta, self.lvl, self.kind, self.want_div, self.want_tv)


def w_rel_term(mrw, term, zero):
    return mrw * term / (zero + EPS)


def w_loss_weights(ep, mrw, R, c0, zc, d0, hw):
    return (-ep.alpha * mrw / (R * (c0 + EPS)), -ep.beta * mrw / (R * (zc + EPS)), ep.delta * mrw / (R * (d0 + EPS) * hw))


def w_mse(s, sE, sEE, HW):
    m, _, D, _, _, sI, sII, sEI = s[:8]
    a = m / D
    return (sEE + HW * a * a + sII / (D * D) + 2.0 * a * sE - 2.0 * sEI / D - 2.0 * a * sI / D) / HW


def w_tv_reported(ep, tv):
    return (tv if ep.want_tv else NAN) if ep.lvl <= 0 else 0.0


def w_terms_of(ep, wc, r, corr, cgm, var, div):
    con, c0 = (var, wc['c0v']) if ep.kind == 1 else (cgm, wc['c0g'])
    return dict(corr=corr, cgm=cgm, var=var, div=div, rel_con=w_rel_term(wc['mrw'][r], con, c0),
                rel_corr=w_rel_term(wc['mrw'][r], corr, wc['zc'][r]), rel_div=w_rel_term(wc['mrw'][r], div, wc['d0']) if ep.want_div else 0.0)


def w_terms_img(ep, wc, r, s, g2, dsum, HW):
    mse = w_mse(s, wc['sE'][r], wc['sEE'][r], HW)
    mean = s[5] / HW
    var = s[6] / HW - mean * mean
    return w_terms_of(ep, wc, r, -mse, g2 / HW, var, dsum / HW if ep.want_div else NAN)


def w_assemble(ep, R, sc, sr, mrd, tv, bad, direct):
    """(value, mean_rel_corr, mean_rel_contrast, mean_rel_div, tv, nonfinite)"""
    mrc, mrr = sc / float(R), sr / float(R)
    val = ep.alpha * (-mrc) + ep.beta * (-mrr)
    if direct:
        if ep.want_tv and ep.gamma != 0.0:
            val += ep.gamma * tv
    else:
        reg = 0.0
        if ep.gamma != 0.0:
            reg += ep.gamma * (tv if ep.lvl <= 0 else 0.0)
        if ep.delta != 0.0:
            reg += ep.delta * mrd
        val += reg
    if bad:
        val = NAN
    return [val, mrr, mrc, mrd, tv, 0.0 if math.isfinite(val) else 1.0]


def w_sum4(p, n):
    ax, ay = [0.0] * 4, [0.0] * 4
    k = 0
    while k + 4 <= n:
        for j in range(4):
            ax[j] += p[2 * (k + j)]
            ay[j] += p[2 * (k + j) + 1]
        k += 4
    while k < n:
        ax[0] += p[2 * k]
        ay[0] += p[2 * k + 1]
        k += 1
    return [(ax[0] + ax[1]) + (ax[2] + ax[3]), (ay[0] + ay[1]) + (ay[2] + ay[3])]


def wc_tokens(wc, R):
    return (wc['c0g'], wc['c0v'], wc['d0'], *wc['zc'][:R], *wc['sE'][:R], *wc['sEE'][:R], *wc['mrw'][:R])


def make_wc(rng, R):
    return dict(c0g=float(rng.uniform(0.5, 2.0)), c0v=float(rng.uniform(0.5, 2.0)), d0=float(rng.uniform(0.5, 2.0)),
                zc=(-rng.uniform(0.1, 1.0, R)).tolist(), sE=rng.uniform(10.0, 200.0, R).tolist(), sEE=rng.uniform(10.0, 200.0, R).tolist(),
                mrw=rng.uniform(0.2, 1.0, R).tolist())


def make_img(rng, HW):
    """The nine image scalars m, M, D, cm, cM, sI, sII, sEI, sG2 of a plausible image."""
    m, M = float(rng.uniform(0.0, 0.1)), float(rng.uniform(0.5, 3.0))
    return [m, M, M - m + EPS, float(rng.integers(1, 5)), float(rng.integers(1, 5)), float(rng.uniform(0.2, 0.6) * HW),
            float(rng.uniform(0.2, 0.6) * HW), float(rng.uniform(0.1, 0.4) * HW), float(rng.uniform(1.0, 50.0) * HW)]


# ================================================================================================
# pinned to the reference
# ================================================================================================
def _fixtures():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'ref_*.npz'))):
        d = np.load(path, allow_pickle=False)
        if 'params' in d.files and 'obj_contrasts' in d.files:
            out.append((os.path.basename(path)[:-4], {k: d[k] for k in d.files if k.startswith('obj_') or k in (
                'params', 'value', 'mean_rel_corr', 'mean_rel_contrast', 'mean_rel_iwe_divergence', 'theta_total_variation')}))
    return out


FIXTURES = _fixtures()
for _name, _d in FIXTURES:
    _a, _b, _g, _dl, _lvl = (float(x) for x in _d['params'])
    _R = len(_d['obj_contrasts'])
    _ep = EP(_a, _b, _g, _dl, _lvl, 0, _dl != 0.0, _lvl <= 0 and _g != 0.0)
    _wc = dict(c0g=float(_d['obj_zero_contrast']), c0v=1.0, d0=float(_d['obj_zero_iwe_divergence']), zc=_d['obj_zero_correlations'].tolist(),
               sE=[0.0] * _R, sEE=[0.0] * _R, mrw=_d['obj_multi_ref_weights'].tolist())
    _per = [x for r in range(_R) for x in (float(_d['obj_contrasts'][r]), float(_d['obj_correlations'][r]), float(_d['obj_iwe_divergences'][r]))]
    _case('ref-' + _name, 'window', *_ep.tokens(), _R, float(_d['theta_total_variation']), 0, 0, *wc_tokens(_wc, _R), *_per)


def test_there_are_fourteen_reference_fixtures():
    assert len(FIXTURES) == 14


@pytest.mark.parametrize('name', [n for n, _ in FIXTURES])
def test_recorded_per_image_values_give_the_recorded_loss(out, name):
    d = dict(FIXTURES)[name]
    got = HC.f(out['ref-' + name][0])
    value, mrr, mrc, mrd = got[:4]
    err = {'value': abs(value - d['value']) / abs(d['value']), 'mean_rel_corr': abs(mrr - d['mean_rel_corr']) / abs(d['mean_rel_corr']),
           'mean_rel_contrast': abs(mrc - d['mean_rel_contrast']) / abs(d['mean_rel_contrast'])}
    if float(d['params'][3]) != 0.0:
        err['mean_rel_iwe_divergence'] = abs(mrd - d['mean_rel_iwe_divergence']) / abs(d['mean_rel_iwe_divergence'])
    print(name, {k: f'{v:.2e}' for k, v in err.items()})
    for k, v in err.items():
        assert v <= 1e-12, (k, v)


# ================================================================================================
# witness, bit for bit: windows over R, contrast kind, delta, level, TV, a NaN theta
# ================================================================================================
WINDOWS = []
_rng = np.random.default_rng(2024)
for _R in (1, 3, 16):
    for _kind in (0, 1):
        for _delta in (0.0, 0.7):
            for _lvl, _gamma, _want_tv in ((0, 2.5e-3, 1), (0, 0.0, 0), (2, 2.5e-3, 0), (0, 0.0, 1)):
                for _bad, _direct in ((0, 0), (1, 0), (0, 1)):
                    if _direct and _delta != 0.0:
                        continue                # (host assembly has no divergence term)
                    _ep = EP(20.0, 35.0, _gamma, _delta, _lvl, _kind, _delta != 0.0, _want_tv)
                    _wc = make_wc(_rng, _R)
                    _per = _rng.uniform(0.1, 2.0, (_R, 3)) * np.array([1.0, -1.0, 1.0])
                    _tv = float(_rng.uniform(1.0, 9.0))
                    _n = _case(f'window-R{_R}-k{_kind}-d{_delta}-l{_lvl}-g{_gamma}-tv{_want_tv}-bad{_bad}-dir{_direct}', 'window', *_ep.tokens(), _R, _tv,
                               _bad, _direct, *wc_tokens(_wc, _R), *_per.reshape(-1).tolist())
                    WINDOWS.append((_n, _ep, _R, _tv, _bad, _direct, _wc, _per.tolist()))


def w_window(ep, R, tv, bad, direct, wc, per):
    sc = sr = sd = 0.0
    cols = []
    for r in range(R):
        con, corr, div = per[r]
        t = w_terms_of(ep, wc, r, -(-corr), con, con, div if ep.want_div else NAN)
        cols.append(t)
        sc += t['rel_con']
        sr += t['rel_corr']
        sd += t['rel_div']
    head = w_assemble(ep, R, sc, sr, sd / float(R) if ep.want_div else NAN, w_tv_reported(ep, tv), bad, direct)
    return head + [t[k] for k in ('corr', 'cgm', 'var', 'div') for t in cols]


def test_windows_equal_the_witness_bit_for_bit(out):
    assert len(WINDOWS) == 3 * 2 * (4 * 3 + 4 * 2)
    for name, *args in WINDOWS:
        assert same_bits(HC.f(out[name][0]), w_window(*args)), name


IMAGES = []
for _k in range(12):
    _ep = EP(20.0, 35.0, 0.0, 0.7 * (_k % 2), 0, (_k // 2) % 2, _k % 2, 0)
    _wc = make_wc(_rng, 1)
    _HW = float(37 * 53)
    _s = make_img(_rng, _HW)
    _g2, _ds = float(_rng.uniform(1.0, 50.0) * _HW), float(_rng.uniform(0.1, 2.0) * _HW)
    IMAGES.append((_case(f'image-{_k}', 'image', *_ep.tokens(), *wc_tokens(_wc, 1), *_s, _g2, _ds, _HW), _ep, _wc, _s, _g2, _ds, _HW))


def test_image_front_ends_pack_and_mse_equal_the_witness(out):
    for name, ep, wc, s, g2, ds, HW in IMAGES:
        t = w_terms_img(ep, wc, 0, s, g2, ds, HW)
        assert same_bits(HC.f(out[name][0]), [t[k] for k in ('corr', 'cgm', 'var', 'div', 'rel_con', 'rel_corr', 'rel_div')]), name
        assert same_bits(HC.f(out[name][1]), s[:8] + [-7.0, 0.0]), name            # pack leaves slot 8 alone; unpack gives sG2 = 0
        assert same_bits(HC.f(out[name][2]), [w_mse(s, wc['sE'][0], wc['sEE'][0], HW)]), name
        assert same_bits(HC.f(out[name][3]), [w_rel_term(wc['mrw'][0], g2, wc['c0v']), w_rel_term(wc['mrw'][0], ds, wc['zc'][0]),
                                               w_rel_term(wc['mrw'][0], g2, ds)]), name


WEIGHTS = []
for _k in range(8):
    _ep = EP(20.0, 35.0, 0.0, 0.7 * (_k % 2), 0, 0, _k % 2, 0)
    _args = (float(_rng.uniform(0.2, 1.0)), float((1, 3, 16)[_k % 3]), float(_rng.uniform(0.5, 2.0)), -float(_rng.uniform(0.1, 1.0)),
             float(_rng.uniform(0.5, 2.0)), (1.0, float(37 * 53))[_k % 2])
    WEIGHTS.append((_case(f'weights-{_k}', 'weights', *_ep.tokens(), *_args), _ep, _args))
TVS = []
for _k, (_a, _nz) in enumerate(((0.0, 0.0), (12.5, 1961.0), (3.0e-7, 1.0), (7.25, 3.0))):
    for _lvl, _want in ((0, 1), (0, 0), (3, 0)):
        _ep = EP(20.0, 35.0, 2.5e-3, 0.0, _lvl, 0, 0, _want)
        TVS.append((_case(f'tv-{_k}-{_lvl}-{_want}', 'tv', *_ep.tokens(), _a, _nz), _ep, _a, _nz))


def test_weights_and_tv_equal_the_witness(out):
    for name, ep, args in WEIGHTS:
        assert same_bits(HC.f(out[name][0]), w_loss_weights(ep, *args)), name
    for name, ep, a, nz in TVS:
        tv = a / (nz + EPS)
        assert same_bits(HC.f(out[name][0]), [tv, w_tv_reported(ep, tv), ep.gamma * 0.25 / (nz + EPS)]), name


# ================================================================================================
# loss_weights is the derivative of assemble_window's value in each image's term
# ================================================================================================
# A quotient of differences carries the rounding of the two values: about k / 2 ulp(v) for the k roundings between the perturbed term and
# the value, against a change of f * 2^-20 * |v| where f is the share of the value the perturbed term carries: k * 1.2e-10 / f
# relative.  So each case makes its term carry the value (f > 0.98): only the perturbed family's coefficient is non-zero and the other
# images' weights are 2^-10; the regularisers are off unless the divergence is the term.  k is the multiply and the divide of
# rel_term, the adds of the sum that still round, the division by R and the product with the coefficient: a handful, so 1e-9 holds.
DERIV = []
for _R in (1, 3, 16):
    _wc0 = make_wc(_rng, _R)
    _per = _rng.uniform(0.5, 2.0, (_R, 3)) * np.array([1.0, -1.0, 1.0])
    for _r in sorted({0, _R // 2, _R - 1}):
        _wc = dict(_wc0, mrw=[1.0 if r == _r else 2.0 ** -10 for r in range(_R)])
        for _j in range(3):
            _ep = EP(20.0 if _j == 0 else 0.0, 35.0 if _j == 1 else 0.0, 0.0, 0.7 if _j == 2 else 0.0, 0, 0, _j == 2, 0)
            _base = ('window', *_ep.tokens(), _R, 4.0, 0, 0, *wc_tokens(_wc, _R))
            _p = _per.copy()
            _p[_r, _j] += float(_p[_r, _j]) * 2.0 ** -20
            _h = float(_p[_r, _j] - _per[_r, _j])           # the perturbation as it was applied
            DERIV.append((_case(f'deriv-R{_R}-r{_r}-t{_j}-base', *_base, *_per.reshape(-1).tolist()),
                          _case(f'deriv-R{_R}-r{_r}-t{_j}', *_base, *_p.reshape(-1).tolist()),
                          _case(f'deriv-R{_R}-r{_r}-t{_j}-w', 'weights', *_ep.tokens(), 1.0, float(_R), _wc['c0g'], _wc['zc'][_r], _wc['d0'], 1.0), _j, _h))


def test_loss_weights_are_the_derivative_of_the_forward_terms(out):
    assert len(DERIV) == (1 + 3 + 3) * 3
    for base, pert, w, j, h in DERIV:
        v0, v1 = HC.f(out[base][0])[0], HC.f(out[pert][0])[0]
        weight = HC.f(out[w][0])[j]
        err = abs((v1 - v0) / h - weight) / abs(weight)
        print(pert, f'{err:.2e}')
        assert err <= 1e-9, (pert, err, (v1 - v0) / h, weight)


# ================================================================================================
# sum_partials_4, copy_scan_finite, the handover
# ================================================================================================
SUMS = []
for _n in list(range(10)) + [4001]:
    _p = (_rng.normal(size=2 * _n) * 10.0 ** _rng.integers(-3, 4, 2 * _n)).tolist()
    SUMS.append((_case(f'sum4-{_n}', 'sum4', _n, *_p), _p, _n))


def test_sum_partials_4_adds_in_its_four_chains(out):
    for name, p, n in SUMS:
        assert same_bits(HC.f(out[name][0]), w_sum4(p, n)), name


SCANS = []
SPECIALS = {'nan': NAN, '+inf': float('inf'), '-inf': float('-inf'), 'denormal': 5e-324, '-0': -0.0}
for _n in (0, 1, 7, 8, 9, 64):
    for _dst in (0, 1):
        _src = _rng.normal(size=_n).tolist()
        SCANS.append((_case(f'scan-{_n}-{_dst}-plain', 'scan', _n, _dst, *_src), _src, _dst, False))
        for _tag, _v in SPECIALS.items():
            for _pos in range(_n):
                _s = list(_src)
                _s[_pos] = _v
                SCANS.append((_case(f'scan-{_n}-{_dst}-{_tag}-{_pos}', 'scan', _n, _dst, *_s), _s, _dst, _tag in ('nan', '+inf', '-inf')))


def test_copy_scan_finite_finds_every_nonfinite_and_copies_exactly(out):
    for name, src, dst, bad in SCANS:
        assert HC.f(out[name][0]).tolist() == [1.0 if bad else 0.0], name
        assert same_bits(HC.f(out[name][1]), src if dst else [-1.0] * len(src)), name


HANDOVERS = []
for _B, _nth in ((1, 2), (3, 32), (2, 2 * 37 * 53)):
    _a = _rng.uniform(0.0, 1.0, _B)
    _prev, _th, _g = (_rng.normal(size=(_B, _nth)) * 3.0 for _ in range(3))
    HANDOVERS.append((_case(f'handover-{_B}-{_nth}', 'handover', _B, _nth, *_a.tolist(), *_prev.reshape(-1).tolist(), *_th.reshape(-1).tolist(),
                            *_g.reshape(-1).tolist()), _a.tolist(), _prev.tolist(), _th.tolist(), _g.tolist()))


def test_handover_blend_and_chain_rule_equal_the_witness(out):
    for name, a, prev, th, g in HANDOVERS:
        blend = [a[b] * prev[b][i] + (1.0 - a[b]) * th[b][i] for b in range(len(a)) for i in range(len(th[b]))]
        chain = []
        for b in range(len(a)):
            s = 0.0
            for i in range(len(th[b])):
                s += g[b][i] * (prev[b][i] - th[b][i])
            chain.append(s)
        assert same_bits(HC.f(out[name][0]), blend) and same_bits(HC.f(out[name][1]), chain), name


# ================================================================================================
# whole evaluations through host_assemble / f64_assemble / obj_assemble and hand_over: three windows, one of them sat out or without
# events, a NaN in one theta
# ================================================================================================
ASSEMBLE = []
_H, _W, _NIG, _NT = 37, 53, 4, 4
_NWG = (_NIG + IG_WAVES - 1) // IG_WAVES
for _mode in (0, 1, 2, 3):
    for _R in (1, 3, 16):
        for _variant in range(4):
            _two = int(_variant % 2 == 0 and not (_mode & 1))
            _nth = 2 if _two else 8
            _delta = 0.7 if (_mode & 1) and _variant >= 2 else 0.0
            _lvl, _gamma, _want_tv = ((0, 2.5e-3, 1), (2, 0.0, 0), (0, 0.0, 0), (0, 2.5e-3, 1))[_variant]
            _ep = EP(20.0, 35.0, _gamma, _delta, _lvl, _variant % 2, _delta != 0.0, _want_tv)
            _wmask = (0b111, 0b101, 0b111, 0b110)[_variant]
            _wins = []
            for _b in range(3):
                _nev = 0 if (_b == 1 and _variant == 2) else 100 + _b
                _theta = _rng.normal(size=_nth).tolist()
                if _b == 2 and _variant in (1, 3):
                    _theta[-1] = NAN
                _wins.append(dict(nev=_nev, nitems=(3, 0, 5)[_b] if _nev else 0, theta=_theta, wc=make_wc(_rng, _R),
                                  c0=_rng.uniform(0.5, 2.0, 4).tolist(), zck=(-_rng.uniform(0.1, 1.0, (4, _R))).tolist(),
                                  tvp=_rng.uniform(0.0, 30.0, _NT * 3).tolist(),
                                  imgs=[dict(s=make_img(_rng, float(_H * _W)), g2=_rng.uniform(1.0, 50.0, _NWG).tolist(),
                                             f64=_rng.uniform(0.1, 2.0, 4).tolist(), ov=[float(_rng.uniform(0.1, 2.0)), -float(_rng.uniform(0.1, 2.0))])
                                        for _ in range(_R)]))
            _g11 = _rng.normal(size=sum(w['nitems'] for w in _wins) * _R * 2).tolist()
            _tok = [_mode, *_ep.tokens(), _R, 3, _wmask, _H, _W, _NIG, _NT, _two, _nth, 2, 3]
            for _w in _wins:
                _tok += [_w['nev'], _w['nitems'], *_w['theta'], *wc_tokens(_w['wc'], _R), *_w['c0'], *[x for row in _w['zck'] for x in row], *_w['tvp']]
                for _im in _w['imgs']:
                    _tok += [*_im['s'], *_im['g2'], *_im['f64'], *_im['ov']]
            ASSEMBLE.append((_case(f'assemble-m{_mode}-R{_R}-v{_variant}', 'assemble', *_tok, *_g11), _mode, _ep, _R, _wmask, _two, _nth, _wins, _g11))


def w_evaluation(mode, ep, R, wmask, two, nth, wins, g11):
    """[[nonfinite], then per window: value and aux, the result block, the gradient]"""
    HW = float(_H * _W)
    parts, nonfinite, item0 = [], False, 0
    for b, w in enumerate(wins):
        sat_out = not (wmask >> b) & 1
        bad = any(not math.isfinite(x) for x in w['theta'])
        grad = [5.0] * nth
        a = nz = 0.0
        if ep.want_tv:
            for i in range(_NT):
                a += w['tvp'][3 * i]
                nz += w['tvp'][3 * i + 1]
        tv = w_tv_reported(ep, a / (nz + EPS))
        sc = sr = sd = 0.0
        cols = []
        for r, im in enumerate(w['imgs']):
            if mode & 1:
                var, g2m, mse, div = im['f64']
                t = w_terms_of(ep, w['wc'], r, -mse, g2m, var, div if ep.want_div else NAN)
            else:
                g2 = 0.0
                for x in im['g2']:
                    g2 += x
                t = w_terms_img(ep, w['wc'], r, im['s'], g2, 0.0, HW)
            cols.append(t)
            sc += t['rel_con']
            sr += t['rel_corr']
            sd += t['rel_div']
        if mode & 1:
            head = w_assemble(ep, R, sc, sr, sd / float(R) if ep.want_div else NAN, tv, bad, False)
        else:
            head = w_assemble(ep, R, sc, sr, NAN, tv, bad, True)
            if two:
                grad = w_sum4(g11[item0 * R * 2:], w['nitems'] * R)
            elif w['nev'] == 0:
                grad = [0.0] * nth
        if mode & 2:
            sc = sr = 0.0
            for r, im in enumerate(w['imgs']):
                sc += w_rel_term(w['wc']['mrw'][r], im['ov'][0], w['c0'][2])
                sr += w_rel_term(w['wc']['mrw'][r], im['ov'][1], w['zck'][3][r])
            obj_bad = bad if not (mode & 1) else math.isnan(head[0])
            head = w_assemble(ep, R, sc, sr, head[3], head[4], obj_bad, False)
        item0 += w['nitems']
        block = head + [t[k] for k in ('corr', 'cgm', 'var', 'div') for t in cols]
        if sat_out:
            parts += [[NAN] * 6, [0.0] * len(block), [0.0] * nth]
        else:
            parts += [[head[0], head[0], head[1], head[2], head[3], head[4]], block, grad]
            nonfinite = nonfinite or head[5] != 0.0
    return [[1.0 if nonfinite else 0.0]] + parts


def test_whole_evaluations_equal_the_witness_bit_for_bit(out):
    assert len(ASSEMBLE) == 48
    for name, *args in ASSEMBLE:
        want = w_evaluation(*args)
        got = out[name]
        assert len(got) == len(want), name
        for k, (g, w) in enumerate(zip(got, want)):
            assert same_bits(HC.f(g), w), (name, k, HC.f(g), w)


# ================================================================================================
# the window constants of the zero pass and objectives()' block
# ================================================================================================
CONSTANTS = []
for _R in (1, 3, 16):
    _o = _rng.uniform(0.1, 2.0, (_R, 4)) * np.array([-1.0, 1.0, 1.0, 1.0])
    _tvp, _mrw, _tv = _rng.uniform(0.0, 30.0, _NT * 3).tolist(), _rng.uniform(0.2, 1.0, _R).tolist(), float(_rng.uniform(1.0, 9.0))
    CONSTANTS.append((_case(f'constants-R{_R}', 'constants', _R, _H, _W, _NT, _tv, *_o.reshape(-1).tolist(), *_tvp, *_mrw), _R, _tv, _o.tolist(), _tvp, _mrw))


def test_window_constants_and_objectives_block_equal_the_witness(out):
    for name, R, tv, o, tvp, mrw in CONSTANTS:
        corr, cgm, var, div = ([row[k] for row in o] for k in range(4))
        c0g, c0v, d0 = cgm[0], var[0], div[0]
        assert same_bits(HC.f(out[name][0]), [c0g, c0v, d0, 1.0 / (c0g + EPS), 1.0 / (c0v + EPS)] + corr + [1.0 / (z + EPS) for z in corr]), name
        td = 0.0
        for k in range(_NT):
            td += tvp[3 * k + 2]
        assert same_bits(HC.f(out[name][1]), [float(R), c0g, c0v, d0, tv, td / (float(_H) * _W)]), name
        assert same_bits(HC.f(out[name][2]), corr + corr + [x / (z + EPS) for x, z in zip(corr, corr)] + cgm + [x / (c0g + EPS) for x in cgm] + div
                         + [x / (d0 + EPS) for x in div] + var + [x / c0v for x in var] + mrw), name
