// The V-cycle's plan (SPEC §S6, §S9): which of a level's vectors every step reads and writes, decided
// in plain C++ before anything is launched, so that tools/cycle_plan_check.cpp can run every plan
// symbolically on the CPU. runtime.hip maps the roles to device pointers and walks the list.
// Point-block smoothing (§S12) takes the same roles as the scalar form: the planner knows two smoother
// families, weighted Jacobi and Chebyshev.
#pragma once
#include <utility>
#include <vector>

namespace pamg {
namespace plan {

// A level's vectors. U0 is level 0's spare vector (the pipeline's second iterate, the Chebyshev cycle's
// fourth ring vector) and exists on level 0 only.
enum Role { NONE = -1, X = 0, B, T, R, U0 };

enum Op {
    SMOOTH_ZERO,   // out = the Jacobi-form step from a zero guess (reads B alone)
    SMOOTH,        // out = the Jacobi-form step from in
    CHEB,          // out = Chebyshev step k from x_k = in and x_{k-1} = xold (NONE: zeros)
    RESID,         // out = B - A in
    JACOBI_RESID,  // out = the Jacobi sweep from in, R = B - A out (the temporally blocked pass)
    RESTRICT,      // B of level + 1 = R_level in
    COARSE,        // out = Ainv in, on the coarsest level
    PROLONG        // out += P_level in, in being a vector of level + 1
};

struct Step {
    int level;
    Op op;
    Role in, xold, out;
    int k;     // CHEB / the Chebyshev family's step 0: the coefficient index; else 0
    int slot;  // profile slot: 0 pre-smoothing, 1 residual, 2 restriction, 3 prolongation, 4 post-smoothing, 5 coarse
};

// The ring slot that holds x_m after a polynomial of degree m (plan_poly's rotation).
inline int poly_last(int m) { return (m - 1) % 3; }

// One Chebyshev polynomial of degree m: the iterates rotate through ring[0..2], x_1 into ring[0],
// x_2 into ring[1], ...: step k writes ring[k % 3], reads x_k = ring[(k - 1) % 3] and x_{k-1} =
// ring[(k - 2) % 3] (k = 1: in, NONE for a zero guess), so out never aliases in or xold as long as the
// three are distinct and `in` is ring[2] or none of them. Returns the role holding x_m.
inline Role plan_poly(int m, Role in, const Role ring[3], int level, int slot, std::vector<Step>& steps) {
    steps.push_back({level, in == NONE ? SMOOTH_ZERO : SMOOTH, in, NONE, ring[0], 0, slot});
    for (int k = 1; k < m; ++k)
        steps.push_back({level, CHEB, ring[(k - 1) % 3], k == 1 ? in : ring[(k - 2) % 3], ring[k % 3], k, slot});
    return ring[poly_last(m)];
}

struct CycleSpec {
    int L = 2;              // levels, >= 2 (one level is the coarse solve alone)
    int nu1 = 1, nu2 = 1;   // V(nu1, nu2): Jacobi sweeps / Chebyshev degrees
    bool cheb = false;      // the Chebyshev family
    bool zero0 = false;     // the level-0 guess is zero
    bool l0_fused = false;  // level 0's one pre-smoothing sweep and its residual are one JACOBI_RESID pass
    // the cross-cycle pipeline's level-0 segments: l0_given - the pre-smoothed iterate is already in
    // l0_t (T or U0) and its residual in R; l0_post - the plan ends with level 0's post-smoothing
    bool l0_given = false;
    Role l0_t = T;
    bool l0_post = true;
};

struct CyclePlan {
    std::vector<Step> steps;
    bool needs_u0 = false;  // some step names U0
    std::vector<Role> res;  // per level: the role holding its result (level 0: X when l0_post)
};

// Weighted Jacobi: the pre-smoothing sweeps ping-pong between T and R and the residual takes the one
// the last sweep left free; the post-smoothing sweeps ping-pong between X and that free one so that
// the last writes X.
// Chebyshev: a polynomial's iterates rotate through the level's X, T and R (X, as x_0 or not yet
// written, is free from step 2 on), so a level >= 1 ends in whichever the degrees select. Level 0 must
// end in X, which the choice of its two rings arranges; from a given guess X is taken as x_0, and U0
// stands in for it where exactly one of the two degrees is a multiple of 3.
inline CyclePlan plan_cycle(const CycleSpec& sp) {
    CyclePlan p;
    const int L = sp.L;
    std::vector<Step>& st = p.steps;
    st.reserve((size_t)(L - 1) * (size_t)(sp.nu1 + sp.nu2 + 3) + 1);
    p.res.assign(L, X);
    std::vector<Role> cur(L, T), spare(L, R);
    const int last1 = poly_last(sp.nu1), last2 = poly_last(sp.nu2);
    for (int l = 0; l < L - 1; ++l) {
        Role c = T, o = R;
        if (l == 0 && sp.l0_given) {
            c = sp.l0_t;
        } else if (sp.cheb) {
            const Role in = l == 0 && !sp.zero0 ? X : NONE;
            Role ring[3] = {T, R, X};
            if (l == 0 && in == X) {
                if (last1 == 2 && last2 != 2) ring[2] = U0;  // x_0 is still read when step nu1 would overwrite it
            } else if (l == 0 && last2 == 2) {
                std::swap(ring[last1], ring[2]);  // the post-smoothing ring ends where it starts: in X
            } else if (l == 0 && last1 == 2) {
                std::swap(ring[0], ring[2]);
            }
            c = plan_poly(sp.nu1, in, ring, l, 0, st);
            o = c == T ? R : T;
        } else if (l == 0 && sp.l0_fused) {
            st.push_back({0, JACOBI_RESID, X, NONE, T, 0, 0});
        } else {
            const bool given = l == 0 && !sp.zero0;
            st.push_back({l, given ? SMOOTH : SMOOTH_ZERO, given ? X : NONE, NONE, c, 0, 0});
            for (int k = 1; k < sp.nu1; ++k) {
                st.push_back({l, SMOOTH, c, NONE, o, 0, 0});
                std::swap(c, o);
            }
        }
        cur[l] = c;
        spare[l] = o;
        const bool have_r = l == 0 && (sp.l0_given || (!sp.cheb && sp.l0_fused));
        if (!have_r) st.push_back({l, RESID, c, NONE, o, 0, 1});
        st.push_back({l, RESTRICT, o, NONE, B, 0, 2});
    }
    st.push_back({L - 1, COARSE, B, NONE, X, 0, 5});
    for (int l = L - 2; l >= 0; --l) {
        const Role c = cur[l];
        st.push_back({l, PROLONG, p.res[l + 1], NONE, c, 0, 3});
        if (l == 0 && !sp.l0_post) {
            p.res[0] = c;
            break;
        }
        if (sp.cheb) {
            // x_0 = c is free again from step 2 on, so it closes the ring behind the level's other two
            // vectors; level 0 puts X where the polynomial ends instead (U0 then fills the ring if
            // that is the slot of c itself)
            const bool end_x = l == 0 && c != X;
            Role ring[3] = {NONE, NONE, c};
            int n = 0;
            for (Role v : {T, R, end_x ? U0 : X})
                if (v != c && n < 2) ring[n++] = v;
            if (end_x && last2 == 2) {
                ring[2] = X;
            } else if (end_x) {
                ring[1 - last2] = ring[0];
                ring[last2] = X;
            }
            p.res[l] = plan_poly(sp.nu2, c, ring, l, 4, st);
        } else {
            Role in = c, sparev = spare[l];
            for (int k = 0; k < sp.nu2; ++k) {
                const Role out = (sp.nu2 - k) % 2 == 1 ? X : sparev;
                st.push_back({l, SMOOTH, in, NONE, out, 0, 4});
                if (out == sparev) sparev = in;
                in = out;
            }
        }
    }
    for (const Step& s : st) p.needs_u0 = p.needs_u0 || s.in == U0 || s.xold == U0 || s.out == U0;
    return p;
}

}  // namespace plan
}  // namespace pamg
