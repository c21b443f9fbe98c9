// The V-cycle planner (csrc/cycle_plan.h) run symbolically on the CPU: every role of every level holds a
// tag saying what value it contains, each step checks the tags it reads and sets the one it writes.
//
//   cycle_plan_check              every plan of L in {2, 3, 4}, nu1, nu2 in 1..64, both families, zero
//                                 guess on / off, and the level-0 segment / fused-pass combinations the
//                                 runtime produces; prints {"plans": N, "bad": M}, exit status 1 if M > 0
//   cycle_plan_check --cases F    for every line of F (tests/golden/cycle_plan_parent.jsonl) the plan of
//                                 that line's case, printed in the same format
//
// Build with -fsanitize=address,undefined (tests/test_cycle_plan_host.py does).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../parallel_amg_amd/csrc/cycle_plan.h"

using namespace pamg::plan;

static const char* kRoleName[] = {"-", "X", "B", "T", "R", "U0"};
static const char* kOpName[] = {"zero", "smooth", "cheb", "resid", "jres", "restrict", "coarse", "prolong"};
static const char* role_name(Role r) { return kRoleName[(int)r + 1]; }

static std::string plan_line(const CycleSpec& sp, const CyclePlan& p) {
    char buf[256];
    snprintf(buf, sizeof buf,
             "{\"L\":%d,\"nu1\":%d,\"nu2\":%d,\"cheb\":%d,\"zero0\":%d,\"fused\":%d,\"given\":\"%s\",\"post\":%d,\"steps\":[",
             sp.L, sp.nu1, sp.nu2, (int)sp.cheb, (int)sp.zero0, (int)sp.l0_fused, sp.l0_given ? role_name(sp.l0_t) : "-",
             (int)sp.l0_post);
    std::string s = buf;
    for (size_t i = 0; i < p.steps.size(); ++i) {
        const Step& t = p.steps[i];
        snprintf(buf, sizeof buf, "%s[%d,\"%s\",\"%s\",\"%s\",\"%s\",%d,%d]", i ? "," : "", t.level, kOpName[t.op],
                 role_name(t.in), role_name(t.xold), role_name(t.out), t.k, t.slot);
        s += buf;
    }
    return s + "]}";
}

// What a vector holds. ITER: iterate k of the level's pre- (phase 0) or post-smoothing (phase 1); the
// post-smoothing's iterate 0 is the prolongation target after the correction was added.
enum Kind { JUNK, RHS, ITER, RESIDUAL, COARSE_SOL };
struct Tag {
    Kind kind = JUNK;
    int phase = 0, k = 0;
    bool is(Kind kd, int ph = 0, int kk = 0) const { return kind == kd && phase == ph && k == kk; }
};

struct Checker {
    const CycleSpec& sp;
    const CyclePlan& p;
    std::vector<std::string> errs;
    std::vector<Tag> tag;                       // L x 5
    std::vector<int> phase, k;                  // per level: the smoothing under way and its newest iterate
    std::vector<int> n_pre, n_post, n_res, n_jres, n_restr, n_prol;
    Checker(const CycleSpec& s, const CyclePlan& pl) : sp(s), p(pl) {}

    Tag& at(int l, Role r) { return tag[(size_t)l * 5 + (int)r]; }
    void err(size_t i, const char* what) { errs.push_back("step " + std::to_string(i) + ": " + what); }
    int nu(int phase_) const { return phase_ == 0 ? sp.nu1 : sp.nu2; }

    void run() {
        const int L = sp.L;
        tag.assign((size_t)L * 5, Tag());
        phase.assign(L, 0);
        k.assign(L, 0);
        for (auto* v : {&n_pre, &n_post, &n_res, &n_jres, &n_restr, &n_prol}) v->assign(L, 0);
        at(0, B).kind = RHS;
        if (!sp.zero0) at(0, X) = {ITER, 0, 0};
        if (sp.l0_given) {  // the chain launch before this plan left the pre-smoothed iterate and its residual
            at(0, X) = Tag();
            at(0, sp.l0_t) = {ITER, 0, sp.nu1};
            at(0, R).kind = RESIDUAL;
            k[0] = sp.nu1;
        }
        bool names_u0 = false;
        for (size_t i = 0; i < p.steps.size(); ++i) {
            const Step& s = p.steps[i];
            const int l = s.level;
            if (l < 0 || l >= L) {
                err(i, "level out of range");
                continue;
            }
            // (a prolongation's in is a vector of level l + 1)
            for (Role r : {s.in, s.xold, s.out})
                if (r == U0) {
                    names_u0 = true;
                    if (l != 0 || (s.op == PROLONG && r == s.in)) err(i, "U0 named outside level 0");
                }
            // aliasing and writes to b
            if (s.op != RESTRICT && s.op != PROLONG) {
                if (s.out == s.in || s.out == s.xold) err(i, "out aliases in or xold");
                if (s.out == B) err(i, "writes the level's b");
            }
            if (s.op == PROLONG && s.out == B) err(i, "writes the level's b");
            if (s.out == NONE) err(i, "no output");
            const bool smoothing = s.op == SMOOTH_ZERO || s.op == SMOOTH || s.op == CHEB || s.op == JACOBI_RESID;
            if (smoothing) {
                if (l >= L - 1) err(i, "smoothing on the coarsest level");
                if (!at(l, B).is(RHS)) err(i, "b is not the right-hand side");
                const int ph = phase[l], kk = k[l];
                if (s.slot != (ph == 0 ? 0 : 4)) err(i, "profile slot");
                if (kk >= nu(ph)) err(i, "more smoothing steps than asked");
                const bool zero_start = ph == 0 && (l > 0 || sp.zero0);
                if (s.op == SMOOTH_ZERO) {
                    if (!(zero_start && kk == 0)) err(i, "zero-guess form where a guess exists");
                    if (s.in != NONE || s.xold != NONE) err(i, "zero-guess form names an input");
                } else {
                    if (kk == 0 && zero_start) err(i, "reads a guess that is zero");
                    else if (s.in == NONE || !at(l, s.in).is(ITER, ph, kk)) err(i, "in does not hold the newest iterate");
                }
                if (s.op == CHEB) {
                    if (!sp.cheb || kk < 1 || s.k != kk) err(i, "Chebyshev step index");
                    if (kk == 1 && zero_start) {
                        if (s.xold != NONE) err(i, "xold named for a zero guess");
                    } else if (s.xold == NONE || !at(l, s.xold).is(ITER, ph, kk - 1)) {
                        err(i, "xold does not hold the iterate before");
                    }
                } else {
                    if (sp.cheb && kk != 0) err(i, "Jacobi-form step inside a polynomial");
                    if (s.k != 0 || s.xold != NONE) err(i, "k / xold on a Jacobi-form step");
                }
                if (s.op == JACOBI_RESID) {
                    if (l != 0 || ph != 0 || sp.nu1 != 1 || s.out != T || s.in == R) err(i, "fused pass out of place");
                    at(0, R) = Tag{RESIDUAL, 0, 0};
                    ++n_jres[l];
                } else {
                    ++(ph == 0 ? n_pre : n_post)[l];
                }
                if (s.out != NONE) at(l, s.out) = {ITER, ph, kk + 1};
                k[l] = kk + 1;
            } else if (s.op == RESID) {
                if (s.slot != 1) err(i, "profile slot");
                if (!at(l, B).is(RHS)) err(i, "b is not the right-hand side");
                if (phase[l] != 0 || s.in == NONE || !at(l, s.in).is(ITER, 0, sp.nu1)) err(i, "residual of something else than the pre-smoothed iterate");
                if (s.out != NONE) at(l, s.out) = Tag{RESIDUAL, 0, 0};
                ++n_res[l];
            } else if (s.op == RESTRICT) {
                if (s.slot != 2) err(i, "profile slot");
                if (l >= L - 1 || s.out != B) err(i, "restriction target");
                else {
                    if (s.in == NONE || !at(l, s.in).is(RESIDUAL)) err(i, "restricts something else than the residual");
                    at(l + 1, B) = Tag{RHS, 0, 0};
                }
                ++n_restr[l];
            } else if (s.op == COARSE) {
                if (s.slot != 5) err(i, "profile slot");
                if (l != L - 1 || s.in != B || s.out != X || !at(l, B).is(RHS)) err(i, "coarse solve");
                at(l, X) = Tag{COARSE_SOL, 0, 0};
            } else if (s.op == PROLONG) {
                if (s.slot != 3) err(i, "profile slot");
                if (l >= L - 1) {
                    err(i, "prolongation from below the coarsest level");
                    continue;
                }
                const Tag& src = s.in == NONE ? Tag() : at(l + 1, s.in);
                if (s.in != p.res[l + 1]) err(i, "reads another role than the plan reports for the level below");
                if (l + 1 == L - 1 ? !src.is(COARSE_SOL) : !src.is(ITER, 1, sp.nu2)) err(i, "the level below is not finished");
                if (phase[l] != 0 || s.out == NONE || !at(l, s.out).is(ITER, 0, sp.nu1)) err(i, "target does not hold the pre-smoothed iterate");
                if (s.out != NONE) at(l, s.out) = {ITER, 1, 0};
                phase[l] = 1;
                k[l] = 0;
                ++n_prol[l];
            } else {
                err(i, "unknown op");
            }
        }
        const size_t end = p.steps.size();
        // where the result lands
        if (sp.l0_post) {
            if (!at(0, X).is(ITER, 1, sp.nu2) || p.res[0] != X) err(end, "level 0 does not end in X");
        } else if (!at(0, p.res[0]).is(ITER, 1, 0)) {
            err(end, "the reported level-0 role does not hold the prolongated iterate");
        }
        if (!at(0, B).is(RHS)) err(end, "level 0's b was written");
        // step counts
        for (int l = 0; l < L - 1; ++l) {
            if (l == 0 && (sp.l0_given || !sp.l0_post)) continue;
            const int f = n_jres[l];
            if (f != (l == 0 && sp.l0_fused ? 1 : 0)) err(end, "fused passes");
            if (n_pre[l] != sp.nu1 - f || n_res[l] != 1 - f || n_restr[l] != 1 || n_prol[l] != 1 || n_post[l] != sp.nu2)
                err(end, "step counts");
        }
        // U0
        if (names_u0 != p.needs_u0) err(end, "needs_u0 differs from the roles named");
        const bool whole = !sp.l0_given && sp.l0_post;
        if (whole && p.needs_u0 != (sp.cheb && !sp.zero0 && ((sp.nu1 % 3 == 0) != (sp.nu2 % 3 == 0))))
            err(end, "needs_u0 differs from the rule");
    }
};

static long g_plans = 0, g_bad = 0;

static void check(const CycleSpec& sp) {
    const CyclePlan p = plan_cycle(sp);
    Checker c(sp, p);
    c.run();
    ++g_plans;
    if (c.errs.empty()) return;
    if (++g_bad <= 10) {
        fprintf(stderr, "%s\n", plan_line(sp, p).c_str());
        for (const std::string& e : c.errs) fprintf(stderr, "  %s\n", e.c_str());
    }
}

static int print_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    std::vector<char> line(1 << 20);
    while (fgets(line.data(), (int)line.size(), f)) {
        CycleSpec sp;
        int cheb = 0, zero0 = 0, fused = 0, post = 1;
        char given[8] = "";
        if (sscanf(line.data(),
                   "{\"L\":%d,\"nu1\":%d,\"nu2\":%d,\"cheb\":%d,\"zero0\":%d,\"fused\":%d,\"given\":\"%3[^\"]\",\"post\":%d,", &sp.L,
                   &sp.nu1, &sp.nu2, &cheb, &zero0, &fused, given, &post) != 8) {
            fprintf(stderr, "bad case line: %.80s\n", line.data());
            fclose(f);
            return 2;
        }
        sp.cheb = cheb;
        sp.zero0 = zero0;
        sp.l0_fused = fused;
        sp.l0_given = strcmp(given, "-") != 0;
        sp.l0_t = strcmp(given, "U0") == 0 ? U0 : T;
        sp.l0_post = post;
        printf("%s\n", plan_line(sp, plan_cycle(sp)).c_str());
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "--cases") == 0) return print_cases(argv[2]);
    // plan_poly alone: the result is the role the last step wrote
    for (int m = 1; m <= 64; ++m)
        for (Role in : {NONE, X}) {
            const Role ring[3] = {T, R, in == X ? X : U0};
            std::vector<Step> st;
            const Role res = plan_poly(m, in, ring, 0, 0, st);
            ++g_plans;
            if ((int)st.size() != m || st.back().out != res) {
                ++g_bad;
                fprintf(stderr, "plan_poly(%d): result role\n", m);
            }
        }
    for (int L = 2; L <= 4; ++L)
        for (int nu1 = 1; nu1 <= 64; ++nu1)
            for (int nu2 = 1; nu2 <= 64; ++nu2)
                for (int cheb = 0; cheb < 2; ++cheb)
                    for (int zero0 = 0; zero0 < 2; ++zero0) {
                        CycleSpec sp;
                        sp.L = L;
                        sp.nu1 = nu1;
                        sp.nu2 = nu2;
                        sp.cheb = cheb;
                        sp.zero0 = zero0;
                        check(sp);
                        // the fused level-0 pass: Jacobi V(1, nu2) from a given guess
                        if (!cheb && !zero0 && nu1 == 1) {
                            sp.l0_fused = true;
                            check(sp);
                            // the cross-cycle pipeline: Jacobi V(1, 1); head, then the steady segments
                            if (nu2 == 1)
                                for (int fused = 0; fused < 2; ++fused) {
                                    sp.l0_fused = fused;
                                    sp.l0_post = false;
                                    sp.l0_given = false;
                                    check(sp);
                                    if (fused) continue;
                                    sp.l0_given = true;
                                    for (Role t0 : {T, U0}) {
                                        sp.l0_t = t0;
                                        check(sp);
                                    }
                                }
                        }
                    }
    printf("{\"plans\": %ld, \"bad\": %ld}\n", g_plans, g_bad);
    return g_bad ? 1 : 0;
}
