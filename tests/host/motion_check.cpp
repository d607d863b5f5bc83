// motion_check — runs the host's rules of the parametric motion-field models (csrc/eincm_motion.h) on the CPU: tests/test_host_motion.py
// builds it with the address and undefined-behaviour sanitizers, hands it a file of cases (one per line: a keyword, then numbers) and
// compares the line it prints for each with numpy, bit for bit.  Nothing of ROCm is included or linked.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_motion.h"

using namespace eincm;

namespace {

struct Args {                       // the numbers of one case, read in order
    std::vector<std::string> tok; size_t k = 1;
    bool more() const { return k < tok.size(); }
    void need() const { if (!more()) { std::fprintf(stderr, "motion_check: '%s' case is short of arguments\n", tok[0].c_str()); std::exit(2); } }
    double f() { need(); return std::strtod(tok[k++].c_str(), nullptr); }
    int i() { need(); return (int)std::strtol(tok[k++].c_str(), nullptr, 10); }
};

void put(double v) { std::printf(" %.17g", v); }

// K cx cy scale, then M (12, K) row major if K is a usable size (otherwise no M follows)
eincm_motion_model read_model(Args& a) {
    eincm_motion_model m{};
    m.n_coeffs = a.i(); m.cx = a.f(); m.cy = a.f(); m.scale = a.f();
    if (m.n_coeffs >= 1 && m.n_coeffs <= MOTION_MAX_K) for (int i = 0; i < MOTION_NQ * m.n_coeffs; ++i) m.M[i] = a.f();
    return m;
}

// model <model>: 0 if it can be used, else 1 and the refusal's words
void model(Args& a) {
    const eincm_motion_model m = read_model(a);
    const char* what = motion_model_error(m);
    std::printf(" %d %s", what ? 1 : 0, what ? what : "ok");
}

// q <model> c[K]: q = M c (12)
void q_of(Args& a) {
    const eincm_motion_model m = read_model(a);
    std::vector<double> c((size_t)m.n_coeffs);
    for (double& v : c) v = a.f();
    double q[MOTION_NQ];
    motion_q(m, c.data(), q);
    for (const double v : q) put(v);
}

// vmax <model> H W c[K]: max|m_j| (6) | the bound of |Theta|
void vmax(Args& a) {
    const eincm_motion_model m = read_model(a);
    const int H = a.i(), W = a.i();
    std::vector<double> c((size_t)m.n_coeffs);
    for (double& v : c) v = a.f();
    double q[MOTION_NQ], mm[MOTION_NM];
    motion_q(m, c.data(), q);
    motion_monomial_bounds(m, H, W, mm);
    for (const double v : mm) put(v);
    std::printf(" |");
    put(motion_abs_bound(q, mm));
}

// sum P parts[P * 12]: mu (12)
void sum(Args& a) {
    const int P = a.i();
    std::vector<double> parts((size_t)P * MOTION_NQ);
    for (double& v : parts) v = a.f();
    double mu[MOTION_NQ];
    motion_sum_partials(parts.data(), P, mu);
    for (const double v : mu) put(v);
}

// project <model> mu[12]: M^T mu (K)
void project(Args& a) {
    const eincm_motion_model m = read_model(a);
    double mu[MOTION_NQ];
    for (double& v : mu) v = a.f();
    std::vector<double> g((size_t)m.n_coeffs);
    motion_project(m, mu, g.data());
    for (const double v : g) put(v);
}

// consts: the sizes the kernels and the host share
void consts(Args&) { std::printf(" %d %d %d %d %d %zu", MOTION_NQ, MOTION_NM, MOTION_MAX_K, MOTION_PARTS, MOTION_ARG_WINDOWS, sizeof(MotionQArg)); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: motion_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "motion_check: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        Args a;
        std::istringstream ss(line);
        for (std::string t; ss >> t; ) a.tok.push_back(t);
        if (a.tok.empty()) continue;
        const std::string& w = a.tok[0];
        std::printf("%s", w.c_str());
        if (w == "model") model(a);
        else if (w == "q") q_of(a);
        else if (w == "vmax") vmax(a);
        else if (w == "sum") sum(a);
        else if (w == "project") project(a);
        else if (w == "consts") consts(a);
        else { std::fprintf(stderr, "motion_check: unknown case '%s'\n", w.c_str()); return 2; }
        if (a.more()) { std::fprintf(stderr, "motion_check: '%s' case has arguments left over\n", w.c_str()); return 2; }
        std::printf("\n");
    }
    return 0;
}
