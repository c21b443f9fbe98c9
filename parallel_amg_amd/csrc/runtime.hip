// runtime.hip — C-ABI implementation of the device side of libpamg (include/pamg.h), all but
// the matrices' upload and layouts (matrix.hip): context and streams, RCCL communicator, exchange
// plans (PartitionedArrays' PRange ghost layout), device vectors, mul!/residual/Jacobi with the
// ghost exchange overlapped with the interior rows, and the V-cycle driver (SPEC.md §S6) replayed
// as a captured hipGraph.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cycle_plan.h"
#include "multi_cols.h"
#include "pamg_device.h"
#include "pamg_host.h"

namespace plan = pamg::plan;

pamg::Options& pamg::options() {
    static Options o;
    return o;
}

// In-process world of sibling contexts (pamg_comm_init_local).
// Ghost exchanges rendezvous PAIRWISE: a part meets only the neighbours its plan lists with a
// non-zero count (so a part with no neighbours, or a decoupled pair of parts, never waits for
// the others — ADVICE r4), and each directed pair carries a sequence number and the plan's tag,
// so two parts whose schedules diverge fail with PAMG_E_STATE instead of exchanging the wrong
// vectors. All-reduce and all-gather are world-wide collectives: every rank
// calls them, they meet at a generation barrier. A failed or abandoned collective marks the
// world broken (every waiting rank fails at once); pamg_world_reset clears that once every rank
// has returned.
struct pamg_world {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool broken = false;
    std::string why;  // first reason the world broke
    int refs = 1;  // the creator's + one per registered context
    struct Slot {
        const double* x = nullptr;        // the posted vector / buffer
        hipEvent_t ready = nullptr;       // recorded after the work that wrote x
        double scalar = 0.0;              // all-reduce operand
    };
    std::vector<Slot> slot;
    // directed pair (q -> p) at index q * n + p: q's post for its exchanges with p
    struct Post {
        uint64_t seq = 0;                 // exchanges q has posted for p so far
        uint64_t read = 0;                // of those, the ones p has finished reading
        const double* x = nullptr;
        const pamg_plan* plan = nullptr;
        hipEvent_t ready = nullptr;
        int64_t tag = 0;
        // q is in (or has made) an exchange under plan tag zero_tag that lists p with zero counts,
        // after zero_at exchanges with p: a p waiting for q's post #zero_at + 1 under the same tag
        // expects a non-zero count — the two parts' plans disagree (fail at once, not
        // after the 300 s timeout)
        uint64_t zero_at = UINT64_MAX;
        int64_t zero_tag = 0;
    };
    std::vector<Post> post;
    std::vector<pamg_ctx*> ctx;
    static constexpr int kTimeoutS = 300;
    void abort_locked(const char* reason) {
        if (!broken) why = reason;
        broken = true;
        cv.notify_all();
    }
    void abort(const char* reason) {
        std::lock_guard<std::mutex> lk(mu);
        abort_locked(reason);
    }
    // wait (lock held) until pred() or the world breaks; false on a break or timeout
    template <class P>
    bool wait_locked(std::unique_lock<std::mutex>& lk, P pred, const char* what) {
        if (broken) return false;
        if (!cv.wait_for(lk, std::chrono::seconds(kTimeoutS), [&] { return pred() || broken; })) {
            abort_locked(what);
            return false;
        }
        return !broken;
    }
    // false when a rank does not come within 300 s (or the world broke): every waiting rank
    // then fails instead of hanging
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const uint64_t g = gen;
        if (++arrived == n) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        return wait_locked(lk, [&] { return gen != g; }, "a rank did not arrive at a collective within 300 s");
    }
    void release() {
        bool last;
        {
            std::lock_guard<std::mutex> lk(mu);
            last = --refs == 0;
        }
        if (last) delete this;
    }
};

namespace {

// a synchronous transport (host staging or the in-process world): exchanges complete inside
// the call, so nothing overlaps them and nothing can be graph-captured
bool sync_transport(const pamg_ctx* ctx) { return ctx->host_fn != nullptr || ctx->world != nullptr; }

// The in-process exchange. For every neighbour q with a non-zero count, part me posts (x, plan,
// tag, ready event) on the pair (me -> q) under the next sequence number, waits for q's post of
// the same number on (q -> me), checks that both posts carry the same tag and matching counts,
// copies the segment q's send list holds for it straight from q's vector into its ghost slots —
// a contiguous run by one copy, any other list by a gather kernel reading the sibling's vector —
// waits for its copies, marks q's post read, and before returning waits until each neighbour has
// read its own post (so x is not written while a sibling still reads it).
int exchange_local(const pamg_plan* plan, double* x, hipStream_t s) {
    pamg_ctx* ctx = plan->ctx;
    pamg_world* w = ctx->world;
    const int me = ctx->rank, nn = (int)plan->nbr.size(), n = w->n;
    std::vector<int> ks, zs;  // neighbours this exchange pairs with; neighbours listed with zero counts
    for (int k = 0; k < nn; ++k)
        (plan->recv_off[k + 1] > plan->recv_off[k] || plan->send_off[k + 1] > plan->send_off[k] ? ks : zs).push_back(k);
    if (!zs.empty() && plan->tag != 0) {
        std::lock_guard<std::mutex> lk(w->mu);
        for (int k : zs) {
            pamg_world::Post& p = w->post[(size_t)me * n + plan->nbr[k]];
            p.zero_at = p.seq;
            p.zero_tag = plan->tag;
        }
        w->cv.notify_all();
    }
    if (ks.empty()) return PAMG_OK;
    HIPC(hipEventRecord(ctx->ev_ready, s));
    std::vector<uint64_t> seq(ks.size());
    {
        std::lock_guard<std::mutex> lk(w->mu);
        if (w->broken) return fail(PAMG_E_STATE, "local exchange: the world is broken (%s)", w->why.c_str());
        for (size_t i = 0; i < ks.size(); ++i) {
            pamg_world::Post& p = w->post[(size_t)me * n + plan->nbr[ks[i]]];
            p.x = x;
            p.plan = plan;
            p.ready = ctx->ev_ready;
            p.tag = plan->tag;
            seq[i] = ++p.seq;
        }
        w->cv.notify_all();
    }
    int rc = PAMG_OK;
    for (size_t i = 0; i < ks.size() && rc == PAMG_OK; ++i) {
        const int k = ks[i], q = plan->nbr[k];
        pamg_world::Post sq;
        {
            std::unique_lock<std::mutex> lk(w->mu);
            const pamg_world::Post& pq = w->post[(size_t)q * n + me];
            auto zero_listed = [&] { return plan->tag != 0 && pq.zero_tag == plan->tag && pq.zero_at + 1 == seq[i]; };
            if (!w->wait_locked(lk, [&] { return pq.seq >= seq[i] || zero_listed(); },
                                "a neighbour part did not post its exchange within 300 s"))
                return fail(PAMG_E_STATE, "local exchange: part %d waited for part %d: the world is broken (%s)", me, q,
                            w->why.c_str());
            if (pq.seq < seq[i]) {
                w->abort_locked("exchange count mismatch");
                return fail(PAMG_E_STATE,
                            "local exchange: part %d expects %lld ghosts from part %d and sends it %lld, but part %d's plan "
                            "(tag %lld) lists part %d with zero counts", me,
                            (long long)(plan->recv_off[k + 1] - plan->recv_off[k]), q,
                            (long long)(plan->send_off[k + 1] - plan->send_off[k]), q, (long long)plan->tag, me);
            }
            sq = pq;
            if (sq.seq != seq[i] || sq.tag != plan->tag) {
                w->abort_locked("exchange pairing mismatch");
                return fail(PAMG_E_STATE,
                            "local exchange: part %d's exchange #%llu with part %d (plan tag %lld) met part %d's exchange "
                            "#%llu (plan tag %lld): the parts' schedules diverged", me, (unsigned long long)seq[i], q,
                            (long long)plan->tag, q, (unsigned long long)sq.seq, (long long)sq.tag);
            }
        }
        const pamg_plan* pq = sq.plan;
        int kq = -1;
        for (int j = 0; pq && j < (int)pq->nbr.size(); ++j)
            if (pq->nbr[j] == me) kq = j;
        const int64_t cnt = plan->recv_off[k + 1] - plan->recv_off[k];
        const int64_t scnt = plan->send_off[k + 1] - plan->send_off[k];
        if (kq < 0 || pq->send_off[kq + 1] - pq->send_off[kq] != cnt || pq->recv_off[kq + 1] - pq->recv_off[kq] != scnt) {
            w->abort("exchange count mismatch");
            return fail(PAMG_E_STATE, "local exchange: part %d expects %lld ghosts from part %d, which sends %lld", me,
                        (long long)cnt, q, kq < 0 ? 0LL : (long long)(pq->send_off[kq + 1] - pq->send_off[kq]));
        }
        if (cnt == 0) continue;
        double* dst = x + plan->n_own + plan->recv_off[k];
        if (hipStreamWaitEvent(s, sq.ready, 0) != hipSuccess) {
            rc = fail(PAMG_E_HIP, "local exchange: stream wait failed");
            break;
        }
        if (pq->send_run[kq] >= 0) {
            if (hipMemcpyAsync(dst, sq.x + pq->send_run[kq], sizeof(double) * cnt, hipMemcpyDefault, s) != hipSuccess)
                rc = fail(PAMG_E_HIP, "local exchange: copy from part %d failed", q);
        } else {
            pamg::launch_pack(cnt, pq->d_send_idx + pq->send_off[kq], sq.x, dst, s);
        }
    }
    if (rc == PAMG_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(PAMG_E_HIP, "local exchange: sync failed");
    std::unique_lock<std::mutex> lk(w->mu);
    if (rc != PAMG_OK) {
        w->abort_locked("a part's exchange failed");
        return rc;
    }
    for (size_t i = 0; i < ks.size(); ++i) w->post[(size_t)plan->nbr[ks[i]] * n + me].read = seq[i];
    w->cv.notify_all();
    for (size_t i = 0; i < ks.size(); ++i) {
        const int q = plan->nbr[ks[i]];
        const pamg_world::Post& mine = w->post[(size_t)me * n + q];
        if (!w->wait_locked(lk, [&] { return mine.read >= seq[i]; }, "a neighbour part did not read its exchange within 300 s"))
            return fail(PAMG_E_STATE, "local exchange: part %d waited for part %d to read: the world is broken (%s)", me,
                        q, w->why.c_str());
    }
    return PAMG_OK;
}

// sum of the ranks' *v in rank order, on every rank
int allreduce_local(pamg_ctx* ctx, double* v) {
    pamg_world* w = ctx->world;
    w->slot[ctx->rank].scalar = *v;
    if (!w->barrier()) return fail(PAMG_E_STATE, "local all-reduce: a sibling part did not arrive");
    double sum = 0.0;
    for (int q = 0; q < w->n; ++q) sum += w->slot[q].scalar;
    if (!w->barrier()) return fail(PAMG_E_STATE, "local all-reduce: a sibling part did not arrive");
    *v = sum;
    return PAMG_OK;
}

// every rank's cnt doubles at its src, in rank order, into dst (cnt per rank)
int allgather_local(pamg_ctx* ctx, const double* src, int64_t cnt, double* dst, hipStream_t s) {
    pamg_world* w = ctx->world;
    const int me = ctx->rank;
    w->slot[me].x = src;
    w->slot[me].ready = ctx->ev_ready;
    HIPC(hipEventRecord(ctx->ev_ready, s));
    if (!w->barrier()) return fail(PAMG_E_STATE, "local all-gather: a sibling part did not arrive");
    int rc = PAMG_OK;
    for (int q = 0; q < w->n && rc == PAMG_OK && cnt > 0; ++q) {
        if (hipStreamWaitEvent(s, w->slot[q].ready, 0) != hipSuccess ||
            hipMemcpyAsync(dst + (size_t)q * cnt, w->slot[q].x, sizeof(double) * cnt, hipMemcpyDefault, s) != hipSuccess)
            rc = fail(PAMG_E_HIP, "local all-gather: copy from part %d failed", q);
    }
    if (rc == PAMG_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(PAMG_E_HIP, "local all-gather: sync failed");
    if (!w->barrier() && rc == PAMG_OK) rc = fail(PAMG_E_STATE, "local all-gather: a sibling part did not arrive");
    return rc;
}

// Ghost exchange of plan on stream s: pack own values, grouped RCCL send/recv straight into
// the ghost slots [n_own + recv_off[k], ...).
int exchange_on(const pamg_plan* plan, double* x, hipStream_t s) {
    pamg_ctx* ctx = plan->ctx;
    const int nn = (int)plan->nbr.size();
    if (nn == 0) return PAMG_OK;
    if (!ctx->comm && !sync_transport(ctx))
        return fail(PAMG_E_STATE, "exchange: plan has neighbours but no communicator");
    // debug (SURVEY §5 race detection): NaN in the ghost slots before every exchange, so a
    // row that reads a ghost before the exchange has landed shows up as NaN
    if (pamg::options().poison_ghosts)
        pamg::launch_fill(plan->recv_off[nn], __builtin_nan(""), x + plan->n_own, s);
    if (ctx->world) return exchange_local(plan, x, s);
    // contiguous send lists go straight from x; the others are packed first
    if (!plan->all_contig)
        pamg::launch_pack(plan->send_off[nn], plan->d_send_idx, x, plan->d_sendbuf, s);
    auto send_ptr = [&](int k) -> const double* {
        return plan->send_run[k] >= 0 ? x + plan->send_run[k] : plan->d_sendbuf + plan->send_off[k];
    };
    if (ctx->host_fn) {  // debug transport: synchronous host staging
        const int64_t ns = plan->send_off[nn], nr = plan->recv_off[nn];
        ctx->h_send.resize(ns + 1);
        ctx->h_recv.resize(nr + 1);
        std::vector<int64_t> sc(nn), rc(nn);
        for (int k = 0; k < nn; ++k) {
            sc[k] = plan->send_off[k + 1] - plan->send_off[k];
            rc[k] = plan->recv_off[k + 1] - plan->recv_off[k];
            if (sc[k])
                HIPC(hipMemcpyAsync(ctx->h_send.data() + plan->send_off[k], send_ptr(k),
                                    sizeof(double) * sc[k], hipMemcpyDeviceToHost, s));
        }
        HIPC(hipStreamSynchronize(s));
        if (ctx->host_fn(ctx->host_user, 0, nn, plan->nbr.data(), sc.data(), ctx->h_send.data(), rc.data(),
                         ctx->h_recv.data()) != 0)
            return fail(PAMG_E_RCCL, "exchange: host transport failed");
        if (nr) HIPC(hipMemcpyAsync(x + plan->n_own, ctx->h_recv.data(), sizeof(double) * nr, hipMemcpyHostToDevice, s));
        HIPC(hipStreamSynchronize(s));
        return PAMG_OK;
    }
    NCCLC(ncclGroupStart());
    for (int k = 0; k < nn; ++k) {
        const size_t sc = (size_t)(plan->send_off[k + 1] - plan->send_off[k]);
        const size_t rc = (size_t)(plan->recv_off[k + 1] - plan->recv_off[k]);
        if (sc) NCCLC(ncclSend(send_ptr(k), sc, ncclDouble, plan->nbr[k], ctx->comm, s));
        if (rc) NCCLC(ncclRecv(x + plan->n_own + plan->recv_off[k], rc, ncclDouble, plan->nbr[k], ctx->comm, s));
    }
    NCCLC(ncclGroupEnd());
    return PAMG_OK;
}

// The exchange of x on the comm stream, behind everything already enqueued on the compute
// stream; `done` is recorded after it (the compute stream, or the caller, waits on that).
int exchange_fork(pamg_ctx* ctx, const pamg_plan* plan, double* x, hipEvent_t done) {
    HIPC(hipEventRecord(ctx->ev_fork, ctx->s_comp));
    HIPC(hipStreamWaitEvent(ctx->s_comm, ctx->ev_fork, 0));
    CHECK(exchange_on(plan, x, ctx->s_comm));
    HIPC(hipEventRecord(done, ctx->s_comm));
    return PAMG_OK;
}

// One operation on the compute stream whose input v needs its ghosts: `overlapped()` enqueues the
// work that reads own entries only, `after()` the work that reads ghost slots. With RCCL the
// exchange runs on the comm stream beside `overlapped` and `after` waits for it; a synchronous
// transport exchanges first (nothing to overlap). plan null or without neighbours: no exchange.
template <class F, class G>
int overlap_exchange(pamg_ctx* ctx, const pamg_plan* plan, double* v, F&& overlapped, G&& after) {
    hipStream_t s = ctx->s_comp;
    bool comm = plan && !plan->nbr.empty();
    if (comm && sync_transport(ctx)) {  // debug / in-process transport: exchange first, no overlap
        CHECK(exchange_on(plan, v, s));
        comm = false;
    }
    if (comm) CHECK(exchange_fork(ctx, plan, v, ctx->ev_join));
    overlapped();
    if (comm) HIPC(hipStreamWaitEvent(s, ctx->ev_join, 0));
    after();
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// y = op(A, x[, b]) with x's ghosts exchanged first; interior rows overlap the exchange.
// OP_CHEB (SPEC §S9 step k >= 1): omega is c2, xold the own rows of x_{k-1} (null: zeros); y
// differs from x and xold.
int apply(pamg_ctx* ctx, const pamg_mat* A, int op, double* x, const double* b, double* y,
          double omega, double c1 = 0.0, const double* xold = nullptr) {
    if (op != pamg::OP_CHEB) xold = x;
    else if (A->interior.pnc || A->interior.rpat || (!A->d_diag && A->nrows > 0))
        return fail(PAMG_E_ARG, "chebyshev: a square operator with a nonzero diagonal is needed");
    if (op == pamg::OP_JACOBI && !A->d_diag && A->nrows > 0)
        return fail(PAMG_E_ARG, "jacobi: a square operator with a nonzero diagonal is needed");
    hipStream_t s = ctx->s_comp;
    return overlap_exchange(
        ctx, A->plan, x, [&]() { pamg::launch_set(*A, A->interior, op, x, b, xold, y, omega, s, c1); },
        [&]() { pamg::launch_set(*A, A->boundary, op, x, b, xold, y, omega, s, c1); });
}

// One smoothing step in point-block form (SPEC §S12) on an operator that carries block data: the residual
// b - A x of the layout's own OP_RESID into y (x's ghosts exchanged by apply), then the block pass over
// the own rows turns y into the new iterate in place — or, where the operator's rows are in the block-row
// layout with this block size, one fused launch with the same bits. BM_ZERO reads b alone (no row sums); y
// differs from x and xold.
int block_step(pamg_ctx* ctx, const pamg_mat* A, int mode, double* x, const double* b, const double* xold, double* y,
               double c1, double c2) {
    hipStream_t s = ctx->s_comp;
    if (mode == pamg::BM_ZERO) {
        pamg::launch_block_update(*A, mode, b, nullptr, nullptr, y, 0.0, c2, s);
    } else if (pamg::bsr_fused(*A) && (mode == pamg::BM_JACOBI || mode == pamg::BM_CHEB)) {
        // a block-row operator (no ghost column, so no exchange): the whole sweep in one launch
        pamg::launch_bsr_block(*A, mode, x, b, xold, y, c1, c2, s);
    } else {
        CHECK(apply(ctx, A, pamg::OP_RESID, x, b, y, 0.0));
        pamg::launch_block_update(*A, mode, y, x, xold, y, c1, c2, s);
    }
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// SPEC §S9 coefficients of a degree-m polynomial over [lmax / ratio, lmax]: fp64, one rounded
// operation each, in the order the specification fixes (built with -ffp-contract=off)
constexpr int kChebMaxDeg = 64;
void cheb_coeffs(double lmax, double ratio, int m, double* c1, double* c2) {
    const double lmin = lmax / ratio;
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
    c1[0] = 0.0;
    c2[0] = 1.0 / theta;
    double r = 1.0 / sigma;
    for (int k = 1; k < m; ++k) {
        const double rk = 1.0 / (2.0 * sigma - r);
        c1[k] = rk * r;
        c2[k] = (2.0 * rk) / delta;
        r = rk;
    }
}

// One smoothing step of a plan (cycle_plan.h) on level operator A: the only place that chooses between
// the scalar (SPEC §S3, §S9) and the point-block form (§S12; blk: A carries block data) and among the
// zero-guess, Jacobi and Chebyshev forms. c2 is the Jacobi weight, or the Chebyshev step's c2 with c1
// (0 outside OP_CHEB); in and xold are null where the step names none.
int smooth_step(pamg_ctx* ctx, const pamg_mat* A, bool blk, plan::Op op, double* in, const double* b, const double* xold,
                double* out, double c1, double c2) {
    if (blk) {
        const int mode = op == plan::CHEB ? pamg::BM_CHEB : op == plan::SMOOTH ? pamg::BM_JACOBI : pamg::BM_ZERO;
        return block_step(ctx, A, mode, in, b, xold, out, c1, c2);
    }
    if (op == plan::CHEB) return apply(ctx, A, pamg::OP_CHEB, in, b, out, c2, c1, xold);
    if (op == plan::SMOOTH) return apply(ctx, A, pamg::OP_JACOBI, in, b, out, c2);
    pamg::launch_jacobi_zero(A->nrows, b, A->d_diag, c2, out, ctx->s_comp);
    return PAMG_OK;
}

// One Chebyshev polynomial of degree m from x_0 = x on operator A (SPEC §S9; block: §S12's form), the
// iterates rotating through t1, t2 and x as plan_poly lays out (x_0 is free again from step 2 on).
// *out: the vector holding x_m.
int cheb_poly(pamg_ctx* ctx, const pamg_mat* A, const double* c1, const double* c2, int m, double* x, const double* b,
              double* t1, double* t2, double** out, bool block) {
    double* const vec[5] = {x, const_cast<double*>(b), t1, t2, nullptr};  // by role
    const plan::Role ring[3] = {plan::T, plan::R, plan::X};
    std::vector<plan::Step> steps;
    *out = vec[plan::plan_poly(m, plan::X, ring, 0, 0, steps)];
    for (const plan::Step& st : steps)
        CHECK(smooth_step(ctx, A, block, st.op, vec[st.in], vec[plan::B], st.xold == plan::NONE ? nullptr : vec[st.xold],
                          vec[st.out], c1[st.k], c2[st.k]));
    return PAMG_OK;
}

// S dependent sweeps (S = 2: Jacobi -> residual; S = 3: Jacobi -> Jacobi -> residual, the
// pipeline's chain) on one part of several whose level is a z-slab in the symmetric layout
// (SymDia::tb_part): the blocked pass k_sym_tb<S> covers the output planes that need no ghost
// (S-1 planes in from a neighbour part) and runs while in0's ghosts travel; the set's planes
// next to them then take the separate sweep, the planes with ghost columns (the boundary
// tiles) theirs after the exchange; each later stage exchanges its input's ghosts while the
// set's planes take the separate sweep, then the boundary planes. Every row's value is the
// separate sweeps' (SPEC §S3 bits).
// exch = false (pamg_bench_rowop): the same launches without the exchanges, to time one part's
// kernels alone (the per-part figures of the multi-GPU model)
int sweeps_part(pamg_ctx* ctx, const pamg_mat* A, int S, const double* in0, double* const* out, const double* b,
                double omega, bool exch = true) {
    hipStream_t s = ctx->s_comp;
    const pamg::SymDia& sd = A->sym;
    const int nz = sd.tb.nz;
    const int zlo = sd.part_lo == 0 ? 0 : sd.part_lo + S - 1, zhi = sd.part_hi == nz ? nz : sd.part_hi - (S - 1);
    pamg::TbArgs ta;
    ta.nstages = S;
    ta.last_resid = true;
    ta.in0 = in0;
    for (int q = 0; q < S; ++q) ta.out[q] = out[q];
    ta.b = b;
    ta.omega = omega;
    for (int q = 0; q < S; ++q) {
        const int op = q == S - 1 ? pamg::OP_RESID : pamg::OP_JACOBI;
        const double w = q == S - 1 ? 0.0 : omega;
        double* v = const_cast<double*>(q == 0 ? in0 : out[q - 1]);
        CHECK(overlap_exchange(
            ctx, exch ? A->plan : nullptr, v,
            [&]() {
                if (q == 0) pamg::launch_sym_tb(*A, ta, s);
                // the set's planes next to the neighbour parts, both sides in one launch
                pamg::launch_sym_planes(*A, op, sd.part_lo, zlo, v, b, out[q], w, s, zhi, sd.part_hi);
            },
            [&]() { pamg::launch_rows(*A, A->boundary, op, v, b, v, out[q], w, s); }));
    }
    return PAMG_OK;
}

int jr_part(pamg_ctx* ctx, const pamg_mat* A, double* x, const double* b, double* t, double* r, double omega) {
    double* out[2] = {t, r};
    return sweeps_part(ctx, A, 2, x, out, b, omega);
}

// Which temporally blocked pass (Options::jr_fuse) a Jacobi sweep followed by the residual takes
// on A: 1 — the whole one-part grid stencil in one launch (k_sym_tb, S = 2); 2 — one part of
// several, the blocked pass on the slab's inner planes (jr_part); 0 — none.
int jr_blocked(const pamg_mat* A) {
    if (!pamg::options().jr_fuse || !A->interior.sym) return 0;
    if (A->sym.tb_ok && !(A->plan && !A->plan->nbr.empty())) return 1;
    return A->sym.tb_part ? 2 : 0;
}

// t = the weighted-Jacobi sweep from x, r = b - A t: the blocked pass jr_blocked names, else two
// sweeps; *fused tells which. Enqueued on the compute stream.
int jacobi_residual(pamg_ctx* ctx, const pamg_mat* A, double* x, const double* b, double* t, double* r, double omega,
                    bool* fused) {
    const int blocked = jr_blocked(A);
    *fused = blocked != 0;
    if (blocked == 2) return jr_part(ctx, A, x, b, t, r, omega);
    if (blocked == 1) {
        pamg::TbArgs ta;
        ta.nstages = 2;
        ta.last_resid = true;
        ta.in0 = x;
        ta.out[0] = t;
        ta.out[1] = r;
        ta.b = b;
        ta.omega = omega;
        pamg::launch_sym_tb(*A, ta, ctx->s_comp);
        HIPC(hipGetLastError());
        return PAMG_OK;
    }
    CHECK(apply(ctx, A, pamg::OP_JACOBI, x, b, t, omega));
    return apply(ctx, A, pamg::OP_RESID, t, b, r, 0.0);
}

// Average milliseconds of `reps` calls of once() on stream s, after one warm-up call. once()
// returns a status; the first failure (of a call, an event or a launch) is returned, the events
// destroyed either way.
template <class F>
int time_reps(hipStream_t s, int reps, double* avg_ms, F&& once) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    const int rc = [&]() -> int {
        HIPC(hipEventCreate(&e0));
        HIPC(hipEventCreate(&e1));
        CHECK(once());
        HIPC(hipEventRecord(e0, s));
        for (int k = 0; k < reps; ++k) CHECK(once());
        HIPC(hipEventRecord(e1, s));
        HIPC(hipEventSynchronize(e1));
        HIPC(hipEventElapsedTime(&ms, e0, e1));
        HIPC(hipGetLastError());
        return PAMG_OK;
    }();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    *avg_ms = ms / reps;
    return rc;
}

// The deterministic dot x.y over the own rows of every rank (fixed-grid partials, then the
// cross-rank sum); `partial` enqueues the partials + final kernels (default: launch_dot).
template <class F>
int reduce_with(pamg_ctx* ctx, int64_t n, double* out, F partial) {
    hipStream_t s = ctx->s_comp;
    const int np = pamg::dot_partials(n);
    if (np + 1 > ctx->red_cap) return fail(PAMG_E_STATE, "reduction workspace too small");
    double* res = ctx->d_red + ctx->red_cap - 1;
    partial(np, ctx->d_red, res, s);
    if (ctx->comm && ctx->nranks > 1) NCCLC(ncclAllReduce(res, res, 1, ncclDouble, ncclSum, ctx->comm, s));
    HIPC(hipMemcpyAsync(ctx->h_red, res, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    *out = *ctx->h_red;
    if (ctx->world && ctx->nranks > 1) CHECK(allreduce_local(ctx, out));
    if (ctx->host_fn && ctx->nranks > 1) {
        const int64_t one = 1;
        double sum = 0.0;
        if (ctx->host_fn(ctx->host_user, 2, 1, nullptr, &one, out, &one, &sum) != 0)
            return fail(PAMG_E_RCCL, "allreduce: host transport failed");
        *out = sum;
    }
    return PAMG_OK;
}

int reduce_scalar(pamg_ctx* ctx, int64_t n, const double* x, const double* y, double* out) {
    return reduce_with(ctx, n, out, [&](int np, double* parts, double* res, hipStream_t s) {
        pamg::launch_dot(n, x, y, parts, np, res, s);
    });
}

// The two sums of a SPEC §S10 step after y = A v, with v <- y / diag in the same pass:
// out[0] = sum v_i y_i, out[1] = sum (a_ii v_i) v_i over the own rows — of every rank when
// all_parts (the cross-rank sums of reduce_with), else of this rank alone (a level held whole).
// blk (SPEC §S12): the block form on that operator's data — (D_b v).v and v <- D_b^-1 y.
int lmax_sums(pamg_ctx* ctx, int64_t n, const double* y, const double* diag, double* v, bool all_parts,
              double out[2], const pamg_mat* blk = nullptr) {
    hipStream_t s = ctx->s_comp;
    const int np = pamg::dot_partials(n);
    if (2 * np + 2 > ctx->red_cap) return fail(PAMG_E_STATE, "reduction workspace too small");
    double* res = ctx->d_red + ctx->red_cap - 2;
    if (blk) pamg::launch_lmax_step_block(*blk, y, v, ctx->d_red, np, res, s);
    else pamg::launch_lmax_step(n, y, diag, v, ctx->d_red, np, res, s);
    HIPC(hipGetLastError());
    const bool cross = all_parts && ctx->nranks > 1;
    if (cross && ctx->comm) NCCLC(ncclAllReduce(res, res, 2, ncclDouble, ncclSum, ctx->comm, s));
    HIPC(hipMemcpyAsync(ctx->h_red, res, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    out[0] = ctx->h_red[0];
    out[1] = ctx->h_red[1];
    if (cross && ctx->world) {
        CHECK(allreduce_local(ctx, &out[0]));
        CHECK(allreduce_local(ctx, &out[1]));
    }
    if (cross && ctx->host_fn) {
        const int64_t two = 2;
        double sum[2] = {0.0, 0.0};
        if (ctx->host_fn(ctx->host_user, 2, 1, nullptr, &two, out, &two, sum) != 0)
            return fail(PAMG_E_RCCL, "allreduce: host transport failed");
        out[0] = sum[0];
        out[1] = sum[1];
    }
    return PAMG_OK;
}

}  // namespace

// ------------------------------------------------------------------ hierarchy type

struct pamg_hier {
    pamg_ctx* ctx = nullptr;
    int L = 0;
    std::vector<const pamg_mat*> A, P, R;
    // the operator PCG forms b - A x and A p with (pamg_hier_set_outer; SPEC §S15), or null: A[0]
    const pamg_mat* outer = nullptr;
    std::vector<double> omega;
    // per-level work vectors (level 0: t, r only; x and b belong to the caller)
    std::vector<double*> x, b, t, r;
    std::vector<int64_t> nown;
    // coarsest level
    int64_t nc = 0;
    double* d_ainv = nullptr;          // row-major nc x nc (the ABI hands it over column-major)
    // replicated tail (SPEC §S7 agglomeration): levels >= rep are held whole on every rank;
    // the restriction into level rep yields this rank's rows [coffs[me], coffs[me+1]), which
    // are all-gathered (in blocks of cmax) into the whole vector
    int rep = 0;
    std::vector<int64_t> coffs;        // nranks + 1
    int64_t cmax = 0;                  // max rows per rank of level rep
    double* d_bgather = nullptr;       // nranks * cmax (+ nc scratch for the one-level case)
    double* d_bsend = nullptr;         // cmax
    // graph replay
    bool use_graph = true;
    hipGraphExec_t gexec = nullptr;
    // cross-cycle pipeline (Options::jr_fuse, stationary cycles): head (first cycle without its
    // level-0 post-smoothing), two steady segments (the previous cycle's post-smoothing fused
    // with this cycle's pre-smoothing and residual, then the rest of the cycle; the level-0
    // iterate alternates between t[0] and u0), two tails (the last post-smoothing)
    hipGraphExec_t g_head = nullptr, g_steady[2] = {nullptr, nullptr}, g_tail[2] = {nullptr, nullptr};
    const double* gp_x = nullptr;
    const double* gp_b = nullptr;
    double* u0 = nullptr;
    const double* g_x = nullptr;
    const double* g_b = nullptr;
    bool g_zero0 = false;
    bool graph_failed = false;
    // PCG workspace (level-0 layout, allocated on first use)
    double *pcg_r = nullptr, *pcg_z = nullptr, *pcg_p = nullptr, *pcg_q = nullptr;
    // device-resident PCG (SPEC §S11, pamg_pcg_resident): the scalar block, the r.r history
    // (pcg_hist_cap entries), the pinned {k, done} slot the first half of an iteration copies
    // out, the pinned values the host uploads per solve, the event ring (lookahead + 1), and the
    // two half-iteration graphs, keyed on the device x (gr_x) like g_x
    pamg::PcgScalars* pcg_S = nullptr;
    double* pcg_hist = nullptr;
    int64_t pcg_hist_cap = 0;
    int* pcg_slot = nullptr;
    double* pcg_stage = nullptr;
    std::vector<hipEvent_t> pcg_ev;
    hipGraphExec_t g_pcg[2] = {nullptr, nullptr};
    const double* gr_x = nullptr;
    // several right-hand sides (SPEC §S13): mc_cols-column copies of the per-level work vectors and of
    // PCG's, column c of level l's at base + c * mc_stride[l]; allocated by the first multi-column call,
    // grown when a later call brings more columns. gm_exec: the multi-column cycle's graph, keyed on the
    // level-0 column bases, the column count and the zero-guess flag.
    int mc_cols = 0;
    std::vector<int64_t> mc_stride;
    std::vector<double*> mx, mb, mt, mr;
    double* mu0 = nullptr;
    double *mpcg_r = nullptr, *mpcg_z = nullptr, *mpcg_p = nullptr, *mpcg_q = nullptr;
    hipGraphExec_t gm_exec = nullptr;
    const double* gm_x = nullptr;
    const double* gm_b = nullptr;
    const double* gm_x1 = nullptr;  // (column 1 of either: the strides)
    const double* gm_b1 = nullptr;
    int gm_k = 0;
    bool gm_zero0 = false;
    // level-0 locality permutation (pamg_hier_set_perm): device row i = caller row perm[i];
    // the caller's x and b are gathered into px / pb at entry and x is scattered back at exit
    int* d_perm = nullptr;
    double *px = nullptr, *pb = nullptr;
    // profiling
    int nu1 = 1, nu2 = 1;  // V(nu1, nu2) Jacobi sweeps (SPEC §S6) / Chebyshev degrees (§S9)
    // smoother (pamg_hier_set_smoother): with PAMG_SMOOTHER_CHEBYSHEV level l's polynomial runs over
    // [lmax[l] / ratio, lmax[l]]; c1 / c2: its step coefficients for every degree up to kChebMaxDeg
    // (the coefficients of degree m are the first m)
    int smoother = PAMG_SMOOTHER_JACOBI;
    double cheb_ratio = 4.0;
    std::vector<double> cheb_lmax;
    std::vector<std::vector<double>> cheb_c1, cheb_c2;
    bool prof = false;
    std::vector<hipEvent_t> ev;
    std::vector<std::pair<int, int>> ev_tag;  // (level, op) per event pair
    std::vector<double> prof_ms;              // L * 6
};

namespace {

// All-gather this rank's block of level H->rep (in d_bsend) into the rank blocks of
// d_bgather, then compact them into global order at dst.
int gather_rep(pamg_hier* H, double* dst, hipStream_t s) {
    pamg_ctx* ctx = H->ctx;
    const int nr = (int)H->coffs.size() - 1;
    if (ctx->host_fn) {
        ctx->h_send.resize(H->cmax + 1);
        ctx->h_recv.resize((size_t)nr * H->cmax + 1);
        HIPC(hipMemcpyAsync(ctx->h_send.data(), H->d_bsend, sizeof(double) * H->cmax, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        const int64_t cnt = H->cmax, tot = (int64_t)nr * H->cmax;
        if (ctx->host_fn(ctx->host_user, 1, nr, nullptr, &cnt, ctx->h_send.data(), &tot, ctx->h_recv.data()) != 0)
            return fail(PAMG_E_RCCL, "allgather: host transport failed");
        HIPC(hipMemcpyAsync(H->d_bgather, ctx->h_recv.data(), sizeof(double) * tot, hipMemcpyHostToDevice, s));
    } else if (ctx->world) {
        CHECK(allgather_local(ctx, H->d_bsend, H->cmax, H->d_bgather, s));
    } else {
        NCCLC(ncclAllGather(H->d_bsend, H->d_bgather, (size_t)H->cmax, ncclDouble, ctx->comm, s));
    }
    for (int q = 0; q < nr; ++q) {
        const int64_t c = H->coffs[q + 1] - H->coffs[q];
        if (c)
            HIPC(hipMemcpyAsync(dst + H->coffs[q], H->d_bgather + (size_t)q * H->cmax,
                                sizeof(double) * c, hipMemcpyDeviceToDevice, s));
    }
    return PAMG_OK;
}

// x_L = Ainv b_L. b_L is whole on every rank, except for a one-level hierarchy on several
// ranks (level 0 is the caller's distributed vector): gather it, solve the own rows.
int coarse_solve(pamg_hier* H, const double* bL, double* xL, hipStream_t s) {
    pamg_ctx* ctx = H->ctx;
    const int nr = (int)H->coffs.size() - 1;
    if (H->L > 1 || nr == 1) {
        pamg::launch_dense_gemv(H->nc, H->nc, 0, H->d_ainv, bL, xL, s);
        return PAMG_OK;
    }
    const int me = ctx->rank;
    const int64_t own0 = H->coffs[me], nown = H->coffs[me + 1] - own0;
    HIPC(hipMemcpyAsync(H->d_bsend, bL, sizeof(double) * nown, hipMemcpyDeviceToDevice, s));
    double* full = H->d_bgather + (size_t)nr * H->cmax;
    CHECK(gather_rep(H, full, s));
    pamg::launch_dense_gemv(nown, H->nc, own0, H->d_ainv, full, xL, s);
    return PAMG_OK;
}

struct ProfScope {
    pamg_hier* H;
    int lev, op;
    hipStream_t s;
    ProfScope(pamg_hier* h, int l, int o, hipStream_t st) : H(h), lev(l), op(o), s(st) {
        if (!H->prof) return;
        hipEvent_t e;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, s);
        H->ev.push_back(e);
    }
    ~ProfScope() {
        if (!H->prof) return;
        hipEvent_t e;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, s);
        H->ev.push_back(e);
        H->ev_tag.emplace_back(lev, op);
    }
};

// One V-cycle (SPEC §S6), enqueued on the compute stream; result in x. zero0: the level-0
// initial guess is zero (preconditioner use), so the level-0 pre-smoothing takes the
// zero-guess form too (bit-identical to the full sweep from x = 0, SPEC §S3).
// Level-0 segments of the cross-cycle pipeline (vcycle_raw): given — the level-0 pre-smoothed
// iterate and residual are already in t0 (t[0] or u0) and r[0] (a k_sym_chain launch made them);
// post — whether this call ends with the level-0 post-smoothing (else the prolongated t0 is left
// for the next chain launch). Defaults: one whole cycle.
struct L0Seg {
    bool given = false;
    plan::Role t0 = plan::T;
    bool post = true;
};

bool cheb_kind(const pamg_hier* H) {
    return H->smoother == PAMG_SMOOTHER_CHEBYSHEV || H->smoother == PAMG_SMOOTHER_BLOCK_CHEBYSHEV;
}
// SPEC §S12 "in the cycle": level l smooths in block form under a block smoother where A_l carries block data
bool block_level(const pamg_hier* H, int l) {
    return (H->smoother == PAMG_SMOOTHER_BLOCK_JACOBI || H->smoother == PAMG_SMOOTHER_BLOCK_CHEBYSHEV) &&
           H->A[l]->bs > 1;
}

// The coefficients of smoothing step k on level l: the Jacobi weight, or the level's Chebyshev c1 / c2
void smooth_coeffs(const pamg_hier* H, int l, int k, double* c1, double* c2) {
    *c1 = cheb_kind(H) ? H->cheb_c1[l][k] : 0.0;
    *c2 = cheb_kind(H) ? H->cheb_c2[l][k] : H->omega[l];
}

// What the planner needs to know of this hierarchy and call (cycle_plan.h)
plan::CycleSpec cycle_spec(const pamg_hier* H, bool zero0, const L0Seg& seg = L0Seg{}) {
    plan::CycleSpec sp;
    sp.L = H->L;
    sp.nu1 = H->nu1;
    sp.nu2 = H->nu2;
    sp.cheb = cheb_kind(H);
    sp.zero0 = zero0;
    // level 0, V(1, nu2) from a given guess: the pre-smoothing sweep and the residual in one temporally
    // blocked pass where the operator has one (jacobi_residual; both timed as jacobi_pre)
    sp.l0_fused = H->smoother == PAMG_SMOOTHER_JACOBI && !zero0 && !seg.given && H->nu1 == 1 && jr_blocked(H->A[0]) != 0;
    sp.l0_given = seg.given;
    sp.l0_t = seg.t0;
    sp.l0_post = seg.post;
    return sp;
}

int vcycle_enqueue(pamg_hier* H, double* x, const double* b, bool zero0 = false, L0Seg seg = L0Seg{}) {
    pamg_ctx* ctx = H->ctx;
    hipStream_t s = ctx->s_comp;
    const int L = H->L;
    if (L == 1) {
        ProfScope p(H, 0, 5, s);
        return coarse_solve(H, b, x, s);
    }
    H->x[0] = x;
    H->b[0] = const_cast<double*>(b);
    // which vector every step reads and writes is the plan's business (proved free of aliasing and
    // stale reads by tools/cycle_plan_check.cpp); here the roles become pointers and the steps launches
    const plan::CyclePlan cp = plan::plan_cycle(cycle_spec(H, zero0, seg));
    if (cp.needs_u0 && !H->u0) return fail(PAMG_E_STATE, "vcycle: the cycle lacks its spare level-0 vector");
    auto vec = [&](int l, plan::Role r) -> double* {
        double* const v[5] = {H->x[l], H->b[l], H->t[l], H->r[l], H->u0};
        return r == plan::NONE ? nullptr : v[r];
    };
    std::optional<ProfScope> scope;  // one per run of steps with the same (level, slot)
    const plan::Step* prev = nullptr;
    for (const plan::Step& st : cp.steps) {
        const int l = st.level;
        if (!prev || prev->level != l || prev->slot != st.slot) {
            scope.reset();
            scope.emplace(H, l, st.slot, s);
        }
        prev = &st;
        double* in = vec(l, st.in);
        double* out = vec(l, st.out);
        switch (st.op) {
            case plan::RESID:
                CHECK(apply(ctx, H->A[l], pamg::OP_RESID, in, H->b[l], out, 0.0));
                break;
            case plan::JACOBI_RESID: {
                bool fused = false;
                CHECK(jacobi_residual(ctx, H->A[l], in, H->b[l], out, H->r[l], H->omega[l], &fused));
                break;
            }
            case plan::RESTRICT:
                if (l + 1 == H->rep && ctx->nranks > 1) {  // into the replicated tail
                    CHECK(apply(ctx, H->R[l], pamg::OP_SPMV, in, nullptr, H->d_bsend, 0.0));
                    CHECK(gather_rep(H, H->b[l + 1], s));
                } else {
                    CHECK(apply(ctx, H->R[l], pamg::OP_SPMV, in, nullptr, H->b[l + 1], 0.0));
                }
                break;
            case plan::COARSE:
                CHECK(coarse_solve(H, in, out, s));
                break;
            case plan::PROLONG:
                CHECK(apply(ctx, H->P[l], pamg::OP_PROLONG, vec(l + 1, st.in), nullptr, out, 0.0));
                break;
            default: {
                double c1, c2;
                smooth_coeffs(H, l, st.k, &c1, &c2);
                CHECK(smooth_step(ctx, H->A[l], block_level(H, l), st.op, in, H->b[l], vec(l, st.xold), out, c1, c2));
            }
        }
    }
    scope.reset();
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// Capture what enqueue() puts on stream s into *exec (thread-local mode: other host threads go on
// launching). False if any step fails; *exec is then not to be used.
template <class F>
bool capture_graph(hipStream_t s, F&& enqueue, hipGraphExec_t* exec) {
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    const int rc = enqueue();
    const hipError_t e2 = hipStreamEndCapture(s, &g);
    const bool ok = rc == PAMG_OK && e2 == hipSuccess && g && hipGraphInstantiate(exec, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    return ok;
}

// A failed capture sends the hierarchy to eager launches of the same kernels for good.
void capture_failed(pamg_hier* H, const char* what) {
    (void)hipGetLastError();
    H->use_graph = false;
    H->graph_failed = true;
    fprintf(stderr, "[pamg] %s graph capture failed (%s); using eager launches\n", what, pamg::last_error().c_str());
}

}  // namespace

// ------------------------------------------------------------------ C-ABI

extern "C" {


int pamg_ctx_create(int device, pamg_ctx** out) {
    if (!out) return fail(PAMG_E_ARG, "ctx_create: out is NULL");
    int ndev = 0;
    HIPC(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(PAMG_E_ARG, "ctx_create: device %d of %d", device, ndev);
    auto c = std::make_unique<pamg_ctx>();
    c->device = device;
    HIPC(hipSetDevice(device));
    HIPC(hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&c->s_comm, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    c->red_cap = 2 * 1024 + 2;  // two sets of dot_partials' 1024 partials + two results (lmax_sums)
    CHECK(dalloc(&c->d_red, c->red_cap));
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&c->h_red), 2 * sizeof(double)));
    *out = c.release();
    return PAMG_OK;
}

int pamg_ctx_destroy(pamg_ctx* ctx) {
    if (!ctx) return PAMG_OK;
    ctx_unref(ctx);
    return PAMG_OK;
}

}  // extern "C"

namespace {
// The context's teardown, when its last reference is dropped: the caller's handle
// (pamg_ctx_destroy) and one per plan / vector / matrix / hierarchy made on it. So the handles
// may be destroyed in any order — e.g. by a garbage collector that finalises a context before
// the vectors that referenced it.
void ctx_teardown(pamg_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->s_comp);
    (void)hipStreamSynchronize(ctx->s_comm);
    if (ctx->comm) ncclCommDestroy(ctx->comm);
    if (ctx->world) {
        {
            std::lock_guard<std::mutex> lk(ctx->world->mu);
            ctx->world->ctx[ctx->rank] = nullptr;
        }
        ctx->world->release();
    }
    if (ctx->ev_ready) (void)hipEventDestroy(ctx->ev_ready);
    dfree(ctx->d_red);
    if (ctx->h_red) (void)hipHostFree(ctx->h_red);
    dfree(ctx->d_redk);
    if (ctx->h_redk) (void)hipHostFree(ctx->h_redk);
    for (int k = 0; k < 2; ++k) {
        if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
        if (ctx->stage_done[k]) (void)hipEventDestroy(ctx->stage_done[k]);
    }
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    (void)hipStreamDestroy(ctx->s_comp);
    (void)hipStreamDestroy(ctx->s_comm);
    delete ctx;
}
}  // namespace

void ctx_ref(pamg_ctx* ctx) { ctx->refs.fetch_add(1); }
void ctx_unref(pamg_ctx* ctx) {
    if (ctx->refs.fetch_sub(1) == 1) ctx_teardown(ctx);
}

extern "C" {

int pamg_device_count(int* n) {
    if (!n) return fail(PAMG_E_ARG, "device_count: NULL");
    HIPC(hipGetDeviceCount(n));
    return PAMG_OK;
}

int pamg_ctx_refcount(const pamg_ctx* ctx, int* refs) {
    if (!ctx || !refs) return fail(PAMG_E_ARG, "ctx_refcount: bad args");
    *refs = (int)ctx->refs.load();
    return PAMG_OK;
}

int pamg_ctx_sync(pamg_ctx* ctx) {
    if (!ctx) return fail(PAMG_E_ARG, "ctx_sync: NULL");
    HIPC(hipStreamSynchronize(ctx->s_comm));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_device_sync(int device) {
    HIPC(hipSetDevice(device));
    HIPC(hipDeviceSynchronize());
    return PAMG_OK;
}

int pamg_comm_unique_id(unsigned char id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    NCCLC(ncclGetUniqueId(&u));
    std::memcpy(id, &u, 128);
    return PAMG_OK;
}

int pamg_runtime_versions(int* hip_runtime, int* hip_built, int* rccl_runtime, int* rccl_built) {
    int hv = 0, rv = 0;
    HIPC(hipRuntimeGetVersion(&hv));
    NCCLC(ncclGetVersion(&rv));
    if (hip_runtime) *hip_runtime = hv;
    if (hip_built) *hip_built = HIP_VERSION;
    if (rccl_runtime) *rccl_runtime = rv;
    if (rccl_built) *rccl_built = NCCL_VERSION_CODE;
    return PAMG_OK;
}

int pamg_comm_init(pamg_ctx* ctx, int nranks, int rank, const unsigned char id[128]) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(PAMG_E_ARG, "comm_init: bad args");
    // The RCCL this process resolved librccl.so.1 to must be the one libpamg was compiled
    // against or newer. A host that loaded another ROCm copy first (the torch wheel bundles
    // HIP 7.0 + RCCL 2.26.6 under the same sonames) binds libpamg's RCCL calls to that older
    // library and its HIP runtime; round 1 saw that combination segfault inside the first
    // captured V-cycle ("Library load order"). Refuse it with an error instead.
    {
        int rv = 0;
        NCCLC(ncclGetVersion(&rv));
        if (rv < NCCL_VERSION_CODE) {
            Dl_info di{};
            const char* path = dladdr(reinterpret_cast<void*>(&ncclGetVersion), &di) && di.dli_fname
                                   ? di.dli_fname : "?";
            return fail(PAMG_E_RCCL,
                        "comm_init: RCCL %d loaded from %s is older than the RCCL %d libpamg was built "
                        "against; load libpamg before any other ROCm copy (e.g. before importing torch)",
                        rv, path, NCCL_VERSION_CODE);
        }
    }
    CHECK(set_device(ctx));
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    NCCLC(ncclCommInitRank(&ctx->comm, nranks, u, rank));
    ctx->rank = rank;
    ctx->nranks = nranks;
    return PAMG_OK;
}

int pamg_comm_init_host(pamg_ctx* ctx, int nranks, int rank, pamg_host_comm_fn fn, void* user) {
    if (!ctx || !fn || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(PAMG_E_ARG, "comm_init_host: bad args");
    if (ctx->comm) return fail(PAMG_E_STATE, "comm_init_host: context already has an RCCL communicator");
    ctx->host_fn = fn;
    ctx->host_user = user;
    ctx->rank = rank;
    ctx->nranks = nranks;
    return PAMG_OK;
}

int pamg_world_create(int nparts, pamg_world** out) {
    if (!out || nparts < 1) return fail(PAMG_E_ARG, "world_create: bad args");
    auto w = new pamg_world();
    w->n = nparts;
    w->slot.resize(nparts);
    w->post.resize((size_t)nparts * nparts);
    w->ctx.assign(nparts, nullptr);
    *out = w;
    return PAMG_OK;
}

int pamg_world_destroy(pamg_world* w) {
    if (w) w->release();
    return PAMG_OK;
}

int pamg_world_abort(pamg_world* w) {
    if (!w) return fail(PAMG_E_ARG, "world_abort: NULL");
    w->abort("pamg_world_abort");
    return PAMG_OK;
}

int pamg_world_reset(pamg_world* w) {
    if (!w) return fail(PAMG_E_ARG, "world_reset: NULL");
    std::lock_guard<std::mutex> lk(w->mu);
    w->broken = false;
    w->why.clear();
    w->arrived = 0;
    for (auto& p : w->post) p = pamg_world::Post();
    return PAMG_OK;
}

int pamg_world_state(pamg_world* w, int* broken) {
    if (!w || !broken) return fail(PAMG_E_ARG, "world_state: bad args");
    std::lock_guard<std::mutex> lk(w->mu);
    *broken = w->broken ? 1 : 0;
    return PAMG_OK;
}

int pamg_comm_init_local(pamg_ctx* ctx, pamg_world* w, int rank) {
    if (!ctx || !w || rank < 0 || rank >= w->n) return fail(PAMG_E_ARG, "comm_init_local: bad args");
    if (ctx->comm || ctx->host_fn || ctx->world)
        return fail(PAMG_E_STATE, "comm_init_local: the context already has a transport");
    CHECK(set_device(ctx));
    {
        std::lock_guard<std::mutex> lk(w->mu);
        if (w->ctx[rank]) return fail(PAMG_E_STATE, "comm_init_local: rank %d is taken", rank);
        // siblings on other GPUs read this one's vectors and it reads theirs (peer access; an
        // already enabled pair is fine)
        for (pamg_ctx* o : w->ctx) {
            if (!o || o->device == ctx->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, ctx->device, o->device) != hipSuccess || !can)
                return fail(PAMG_E_HIP, "comm_init_local: devices %d and %d cannot access each other", ctx->device,
                            o->device);
            for (int d = 0; d < 2; ++d) {
                (void)hipSetDevice(d == 0 ? ctx->device : o->device);
                const hipError_t e = hipDeviceEnablePeerAccess(d == 0 ? o->device : ctx->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return fail(PAMG_E_HIP, "comm_init_local: peer access %d <-> %d: %s", ctx->device, o->device,
                                hipGetErrorString(e));
                (void)hipGetLastError();
            }
            CHECK(set_device(ctx));
        }
        w->ctx[rank] = ctx;
        ++w->refs;
    }
    if (!ctx->ev_ready) HIPC(hipEventCreateWithFlags(&ctx->ev_ready, hipEventDisableTiming));
    ctx->world = w;
    ctx->rank = rank;
    ctx->nranks = w->n;
    return PAMG_OK;
}

}  // extern "C"

namespace {
// f(r) for every rank r of w, each on its own host thread (the world's contexts meet inside);
// the first failure's code, with the failing part's message in this thread's error state
template <class F>
int world_each(pamg_world* w, F&& f) {
    if (!w) return fail(PAMG_E_ARG, "world: NULL");
    for (int r = 0; r < w->n; ++r)
        if (!w->ctx[r]) return fail(PAMG_E_STATE, "world: rank %d has no context", r);
    std::vector<int> rc(w->n, PAMG_OK), order(w->n, INT32_MAX);
    std::vector<std::string> msg(w->n);
    std::vector<std::thread> th;
    std::atomic<int> nfail{0};
    for (int r = 0; r < w->n; ++r)
        th.emplace_back([&, r] {
            rc[r] = f(r);
            if (rc[r] != PAMG_OK) {
                msg[r] = pamg::last_error();
                order[r] = nfail.fetch_add(1);
                w->abort("a part's call failed");  // its siblings stop waiting for it now
            }
        });
    for (auto& t : th) t.join();
    if (nfail.load() == 0) return PAMG_OK;
    // the part that failed first (the cause; the others failed because the world broke)
    const int r = (int)(std::min_element(order.begin(), order.end()) - order.begin());
    // every part has returned (the library owns all the world's threads here), so the break
    // that released the siblings is cleared: one part's argument error leaves the world usable
    // for the next call
    (void)pamg_world_reset(w);
    return fail(rc[r], "part %d: %s", r, msg[r].c_str());
}
}  // namespace

extern "C" {

int pamg_world_spmv(pamg_world* w, pamg_mat* const* A, pamg_vec* const* x, pamg_vec* const* y) {
    if (!A || !x || !y) return fail(PAMG_E_ARG, "world_spmv: bad args");
    return world_each(w, [&](int r) { return pamg_spmv(w->ctx[r], A[r], x[r], y[r]); });
}

int pamg_world_exchange(pamg_world* w, pamg_plan* const* plan, pamg_vec* const* x) {
    if (!plan || !x) return fail(PAMG_E_ARG, "world_exchange: bad args");
    return world_each(w, [&](int r) { return pamg_exchange(w->ctx[r], plan[r], x[r]); });
}

int pamg_world_dot(pamg_world* w, pamg_vec* const* x, pamg_vec* const* y, double* out) {
    if (!x || !y || !out || !w) return fail(PAMG_E_ARG, "world_dot: bad args");
    std::vector<double> v(w->n, 0.0);
    CHECK(world_each(w, [&](int r) { return pamg_vec_dot(w->ctx[r], x[r], y[r], &v[r]); }));
    *out = v[0];  // (every rank holds the same sum)
    return PAMG_OK;
}

int pamg_world_vcycle(pamg_world* w, pamg_hier* const* H, pamg_vec* const* x, pamg_vec* const* b, int ncycles,
                      double* res_hist) {
    if (!H || !x || !b || !w) return fail(PAMG_E_ARG, "world_vcycle: bad args");
    // every rank takes the same schedule: with a history each computes the norms (an all-reduce
    // per cycle), so each gets a buffer of its own and rank 0's is returned
    if (ncycles < 0) return fail(PAMG_E_ARG, "world_vcycle: ncycles < 0");
    std::vector<std::vector<double>> hist(w->n, std::vector<double>(res_hist ? (size_t)ncycles : 0));
    CHECK(world_each(w, [&](int r) {
        return pamg_vcycle(w->ctx[r], H[r], x[r], b[r], ncycles, res_hist ? hist[r].data() : nullptr);
    }));
    if (res_hist) std::copy(hist[0].begin(), hist[0].end(), res_hist);
    return PAMG_OK;
}

int pamg_world_pcg(pamg_world* w, pamg_hier* const* H, pamg_vec* const* x, pamg_vec* const* b, double rtol,
                   int maxit, int* iters, double* res_hist) {
    if (!H || !x || !b || !w) return fail(PAMG_E_ARG, "world_pcg: bad args");
    if (maxit < 0) return fail(PAMG_E_ARG, "world_pcg: maxit < 0");
    std::vector<std::vector<double>> hist(w->n, std::vector<double>(res_hist ? (size_t)maxit + 1 : 0));
    std::vector<int> it(w->n, 0);
    CHECK(world_each(w, [&](int r) {
        return pamg_pcg(w->ctx[r], H[r], x[r], b[r], rtol, maxit, &it[r], res_hist ? hist[r].data() : nullptr);
    }));
    if (iters) *iters = it[0];
    if (res_hist) std::copy(hist[0].begin(), hist[0].end(), res_hist);
    return PAMG_OK;
}

int pamg_comm_rank(const pamg_ctx* ctx, int* rank, int* nranks) {
    if (!ctx) return fail(PAMG_E_ARG, "comm_rank: NULL");
    if (rank) *rank = ctx->rank;
    if (nranks) *nranks = ctx->nranks;
    return PAMG_OK;
}

int pamg_plan_create(pamg_ctx* ctx, int64_t n_own, int64_t n_ghost, int n_nbr,
                     const int32_t* nbr_rank, const int64_t* recv_counts,
                     const int64_t* send_counts, const int64_t* send_idx, pamg_plan** out) {
    if (!ctx || !out || n_own < 0 || n_ghost < 0 || n_nbr < 0)
        return fail(PAMG_E_ARG, "plan_create: bad args");
    if (n_nbr > 0 && (!nbr_rank || !recv_counts || !send_counts))
        return fail(PAMG_E_ARG, "plan_create: neighbour arrays missing");
    if (n_own >= INT32_MAX || n_own + n_ghost >= INT32_MAX)
        return fail(PAMG_E_OVERFLOW, "plan_create: sizes exceed int32");
    CHECK(set_device(ctx));
    // released through pamg_plan_destroy on every error path
    std::unique_ptr<pamg_plan, int (*)(pamg_plan*)> p(new pamg_plan, pamg_plan_destroy);
    p->ctx = ctx;
    ctx_ref(ctx);
    p->n_own = n_own;
    p->n_ghost = n_ghost;
    p->nbr.assign(nbr_rank, nbr_rank + n_nbr);
    p->recv_off.assign(n_nbr + 1, 0);
    p->send_off.assign(n_nbr + 1, 0);
    for (int k = 0; k < n_nbr; ++k) {
        // a part may be its own neighbour (ghost copies of own entries, e.g. a periodic wrap
        // on one part): RCCL serves that as a send/recv to self; the host transport does not
        if (nbr_rank[k] < 0 || nbr_rank[k] >= ctx->nranks || (nbr_rank[k] == ctx->rank && ctx->host_fn))
            return fail(PAMG_E_ARG, "plan_create: bad neighbour rank %d", nbr_rank[k]);
        p->recv_off[k + 1] = p->recv_off[k] + recv_counts[k];
        p->send_off[k + 1] = p->send_off[k] + send_counts[k];
    }
    if (p->recv_off[n_nbr] != n_ghost)
        return fail(PAMG_E_ARG, "plan_create: recv counts sum %lld != n_ghost %lld",
                    (long long)p->recv_off[n_nbr], (long long)n_ghost);
    const int64_t ns = p->send_off[n_nbr];
    std::vector<int> idx(ns);
    for (int64_t k = 0; k < ns; ++k) {
        if (send_idx[k] < 0 || send_idx[k] >= n_own)
            return fail(PAMG_E_ARG, "plan_create: send index %lld out of range", (long long)send_idx[k]);
        idx[k] = (int)send_idx[k];
    }
    p->send_run.assign(n_nbr, -1);
    p->all_contig = true;
    for (int k = 0; k < n_nbr; ++k) {
        const int64_t a = p->send_off[k], e = p->send_off[k + 1];
        bool run = e > a;
        for (int64_t j = a + 1; run && j < e; ++j) run = idx[j] == idx[j - 1] + 1;
        if (run) p->send_run[k] = idx[a];
        else if (e > a) p->all_contig = false;
    }
    CHECK(dalloc(&p->d_send_idx, ns));
    CHECK(dalloc(&p->d_sendbuf, ns));
    if (ns) HIPC(hipMemcpy(p->d_send_idx, idx.data(), sizeof(int) * ns, hipMemcpyHostToDevice));
    *out = p.release();
    return PAMG_OK;
}

int pamg_plan_set_tag(pamg_plan* p, int64_t tag) {
    if (!p) return fail(PAMG_E_ARG, "plan_set_tag: NULL");
    p->tag = tag;
    return PAMG_OK;
}

int pamg_plan_destroy(pamg_plan* p) {
    if (!p) return PAMG_OK;
    (void)hipSetDevice(p->ctx->device);
    if (p->in_flight) (void)hipStreamSynchronize(p->ctx->s_comm);
    if (p->ev_done) (void)hipEventDestroy(p->ev_done);
    dfree(p->d_send_idx);
    dfree(p->d_sendbuf);
    pamg_ctx* owner = p->ctx;
    delete p;
    ctx_unref(owner);
    return PAMG_OK;
}

int pamg_vec_create(pamg_ctx* ctx, int64_t n_own, int64_t n_ghost, pamg_vec** out) {
    if (!ctx || !out || n_own < 0 || n_ghost < 0) return fail(PAMG_E_ARG, "vec_create: bad args");
    CHECK(set_device(ctx));
    std::unique_ptr<pamg_vec, int (*)(pamg_vec*)> v(new pamg_vec, pamg_vec_destroy);
    v->ctx = ctx;
    ctx_ref(ctx);
    v->n_own = n_own;
    v->n_ghost = n_ghost;
    v->stride = pamg::mc::col_stride(n_own, n_ghost);
    CHECK(dalloc(&v->d, n_own + n_ghost + kVecPad));
    HIPC(hipMemsetAsync(v->d, 0, sizeof(double) * (n_own + n_ghost + kVecPad), ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    *out = v.release();
    return PAMG_OK;
}

int pamg_vec_destroy(pamg_vec* v) {
    if (!v) return PAMG_OK;
    (void)hipSetDevice(v->ctx->device);
    (void)hipStreamSynchronize(v->ctx->s_comp);
    if (v->owns) dfree(v->d);  // (a column view of a multi-vector owns nothing)
    pamg_ctx* owner = v->ctx;
    delete v;
    ctx_unref(owner);
    return PAMG_OK;
}

int pamg_vec_size(const pamg_vec* v, int64_t* n_own, int64_t* n_ghost) {
    if (!v) return fail(PAMG_E_ARG, "vec_size: NULL");
    if (n_own) *n_own = v->n_own;
    if (n_ghost) *n_ghost = v->n_ghost;
    return PAMG_OK;
}

int pamg_vec_upload(pamg_ctx* ctx, pamg_vec* v, const double* own) {
    if (!ctx || !v || (!own && v->n_own)) return fail(PAMG_E_ARG, "vec_upload: bad args");
    CHECK(set_device(ctx));
    if (v->n_own) HIPC(hipMemcpyAsync(v->d, own, sizeof(double) * v->n_own, hipMemcpyHostToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_download(pamg_ctx* ctx, const pamg_vec* v, double* own) {
    if (!ctx || !v || (!own && v->n_own)) return fail(PAMG_E_ARG, "vec_download: bad args");
    CHECK(set_device(ctx));
    if (v->n_own) HIPC(hipMemcpyAsync(own, v->d, sizeof(double) * v->n_own, hipMemcpyDeviceToHost, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_download_ghosts(pamg_ctx* ctx, const pamg_vec* v, double* ghost) {
    if (!ctx || !v || (!ghost && v->n_ghost)) return fail(PAMG_E_ARG, "vec_download_ghosts: bad args");
    CHECK(set_device(ctx));
    if (v->n_ghost)
        HIPC(hipMemcpyAsync(ghost, v->d + v->n_own, sizeof(double) * v->n_ghost, hipMemcpyDeviceToHost,
                            ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_device_ptr(pamg_vec* v, double** dptr) {
    if (!v || !dptr) return fail(PAMG_E_ARG, "vec_device_ptr: bad args");
    *dptr = v->d;
    return PAMG_OK;
}

int pamg_vec_fill(pamg_ctx* ctx, pamg_vec* v, double value) {
    if (!ctx || !v) return fail(PAMG_E_ARG, "vec_fill: bad args");
    CHECK(set_device(ctx));
    pamg::launch_fill(v->n_own, value, v->d, ctx->s_comp);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_fill_xstar(pamg_ctx* ctx, pamg_vec* v, int64_t i0, uint64_t seed) {
    if (!ctx || !v || i0 < 0) return fail(PAMG_E_ARG, "vec_fill_xstar: bad args");
    CHECK(set_device(ctx));
    pamg::launch_fill_xstar(v->n_own, i0, seed, v->d, ctx->s_comp);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_copy(pamg_ctx* ctx, const pamg_vec* src, pamg_vec* dst) {
    if (!ctx || !src || !dst || src->n_own != dst->n_own) return fail(PAMG_E_ARG, "vec_copy: shape mismatch");
    CHECK(set_device(ctx));
    if (src->n_own)
        HIPC(hipMemcpyAsync(dst->d, src->d, sizeof(double) * src->n_own, hipMemcpyDeviceToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_axpby(pamg_ctx* ctx, double a, const pamg_vec* x, double b, pamg_vec* y) {
    if (!ctx || !x || !y || x->n_own != y->n_own) return fail(PAMG_E_ARG, "vec_axpby: shape mismatch");
    CHECK(set_device(ctx));
    pamg::launch_axpby(x->n_own, a, x->d, b, y->d, ctx->s_comp);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vec_dot(pamg_ctx* ctx, const pamg_vec* x, const pamg_vec* y, double* out) {
    if (!ctx || !x || !y || !out || x->n_own != y->n_own) return fail(PAMG_E_ARG, "vec_dot: shape mismatch");
    CHECK(set_device(ctx));
    return reduce_scalar(ctx, x->n_own, x->d, y->d, out);
}

int pamg_vec_nrm2(pamg_ctx* ctx, const pamg_vec* x, double* out) {
    if (!ctx || !x || !out) return fail(PAMG_E_ARG, "vec_nrm2: bad args");
    CHECK(set_device(ctx));
    double s = 0.0;
    CHECK(reduce_scalar(ctx, x->n_own, x->d, x->d, &s));
    *out = std::sqrt(s);
    return PAMG_OK;
}

int pamg_exchange(pamg_ctx* ctx, const pamg_plan* plan, pamg_vec* x) {
    if (!ctx || !plan || !x) return fail(PAMG_E_ARG, "exchange: bad args");
    if (x->n_own != plan->n_own || x->n_ghost < plan->n_ghost)
        return fail(PAMG_E_ARG, "exchange: vector does not fit the plan");
    CHECK(set_device(ctx));
    CHECK(exchange_on(plan, x->d, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

// consistent!(x) split in two (PartitionedArrays returns a task to wait on): begin forks the
// exchange onto the comm stream behind everything already enqueued on the compute stream and
// returns; end joins it back (later compute-stream work sees the ghosts) and waits for it.
// Between the two the caller may run anything that does not touch x's ghost slots or write
// its send entries. The host debug transport has nothing to overlap: begin does it all.
int pamg_exchange_begin(pamg_ctx* ctx, pamg_plan* plan, pamg_vec* x) {
    if (!ctx || !plan || !x) return fail(PAMG_E_ARG, "exchange_begin: bad args");
    if (x->n_own != plan->n_own || x->n_ghost < plan->n_ghost)
        return fail(PAMG_E_ARG, "exchange_begin: vector does not fit the plan");
    if (plan->in_flight) return fail(PAMG_E_STATE, "exchange_begin: the plan has an exchange in flight");
    CHECK(set_device(ctx));
    if (sync_transport(ctx)) {
        CHECK(exchange_on(plan, x->d, ctx->s_comp));
        plan->in_flight = x;
        return PAMG_OK;
    }
    if (!plan->ev_done) HIPC(hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
    CHECK(exchange_fork(ctx, plan, x->d, plan->ev_done));
    plan->in_flight = x;
    return PAMG_OK;
}

int pamg_exchange_end(pamg_ctx* ctx, pamg_plan* plan, pamg_vec* x) {
    if (!ctx || !plan || !x) return fail(PAMG_E_ARG, "exchange_end: bad args");
    if (plan->in_flight != x) return fail(PAMG_E_STATE, "exchange_end: no exchange of this vector in flight");
    CHECK(set_device(ctx));
    plan->in_flight = nullptr;
    if (!sync_transport(ctx)) {
        HIPC(hipStreamWaitEvent(ctx->s_comp, plan->ev_done, 0));
        HIPC(hipEventSynchronize(plan->ev_done));
    }
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

static int check_vec_for(const pamg_mat* A, const pamg_vec* x, const char* who) {
    const int64_t need_ghost = A->plan ? A->plan->n_ghost : 0;
    const int64_t own = A->plan ? A->plan->n_own : A->ncols;
    if (x->n_own != own || x->n_ghost < need_ghost)
        return fail(PAMG_E_ARG, "%s: input vector (%lld own, %lld ghost) does not fit the matrix columns (%lld own, %lld ghost)",
                    who, (long long)x->n_own, (long long)x->n_ghost, (long long)own, (long long)need_ghost);
    return PAMG_OK;
}

int pamg_spmv(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, pamg_vec* y) {
    if (!ctx || !A || !x || !y) return fail(PAMG_E_ARG, "spmv: NULL");
    CHECK(check_vec_for(A, x, "spmv"));
    if (y->n_own != A->nrows) return fail(PAMG_E_ARG, "spmv: output size mismatch");
    if (x == y) return fail(PAMG_E_ARG, "spmv: x and y must differ");
    CHECK(set_device(ctx));
    CHECK(apply(ctx, A, pamg::OP_SPMV, x->d, nullptr, y->d, 0.0));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_residual(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* r,
                  double* nrm2) {
    if (!ctx || !A || !x || !b || !r) return fail(PAMG_E_ARG, "residual: NULL");
    CHECK(check_vec_for(A, x, "residual"));
    if (b->n_own != A->nrows || r->n_own != A->nrows || r == x)
        return fail(PAMG_E_ARG, "residual: size mismatch or aliasing");
    CHECK(set_device(ctx));
    CHECK(apply(ctx, A, pamg::OP_RESID, x->d, b->d, r->d, 0.0));
    if (nrm2) {
        double s = 0.0;
        CHECK(reduce_scalar(ctx, r->n_own, r->d, r->d, &s));
        *nrm2 = std::sqrt(s);
    }
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_jacobi(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* tmp,
                double omega, int nsweeps) {
    if (!ctx || !A || !x || !b || !tmp || nsweeps < 0) return fail(PAMG_E_ARG, "jacobi: bad args");
    CHECK(check_vec_for(A, x, "jacobi"));
    CHECK(check_vec_for(A, tmp, "jacobi"));
    if (pamg::bsr_any(*A) && A->nrows != (A->plan ? A->plan->n_own : A->ncols))
        return fail(PAMG_E_ARG, "jacobi: the block-row operator must be square (%lld rows, %lld own columns)",
                    (long long)A->nrows, (long long)(A->plan ? A->plan->n_own : A->ncols));
    if (!A->d_diag) return fail(PAMG_E_SETUP, "jacobi: matrix is not square or lacks a nonzero diagonal");
    if (b->n_own != A->nrows || tmp == x) return fail(PAMG_E_ARG, "jacobi: size mismatch or aliasing");
    CHECK(set_device(ctx));
    double* cur = x->d;
    double* nxt = tmp->d;
    for (int k = 0; k < nsweeps; ++k) {
        CHECK(apply(ctx, A, pamg::OP_JACOBI, cur, b->d, nxt, omega));
        std::swap(cur, nxt);
    }
    if (cur != x->d)
        HIPC(hipMemcpyAsync(x->d, cur, sizeof(double) * x->n_own, hipMemcpyDeviceToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_jacobi_residual(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* t,
                         pamg_vec* r, double omega, int* fused) {
    if (!ctx || !A || !x || !b || !t || !r) return fail(PAMG_E_ARG, "jacobi_residual: NULL");
    CHECK(check_vec_for(A, x, "jacobi_residual"));
    CHECK(check_vec_for(A, t, "jacobi_residual"));
    if (pamg::bsr_any(*A) && A->nrows != (A->plan ? A->plan->n_own : A->ncols))
        return fail(PAMG_E_ARG, "jacobi_residual: the block-row operator must be square (%lld rows, %lld own columns)",
                    (long long)A->nrows, (long long)(A->plan ? A->plan->n_own : A->ncols));
    if (!A->d_diag) return fail(PAMG_E_SETUP, "jacobi_residual: matrix is not square or lacks a nonzero diagonal");
    if (b->n_own != A->nrows || r->n_own != A->nrows || t == x || r == x || r == t || b == t || b == r)
        return fail(PAMG_E_ARG, "jacobi_residual: size mismatch or aliasing");
    CHECK(set_device(ctx));
    bool did_fuse = false;
    CHECK(jacobi_residual(ctx, A, x->d, b->d, t->d, r->d, omega, &did_fuse));
    if (fused) *fused = did_fuse ? 1 : 0;
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_hier_create(pamg_ctx* ctx, int nlevels, pamg_mat* const* A, pamg_mat* const* P,
                     pamg_mat* const* R, const double* omega, int64_t n_coarse,
                     const double* ainv, int rep_level, const int64_t* rep_offsets,
                     pamg_hier** out) {
    if (!ctx || !out || nlevels < 1 || !A || !omega || !ainv || n_coarse < 1)
        return fail(PAMG_E_ARG, "hier_create: bad args");
    if (nlevels > 1 && (!P || !R)) return fail(PAMG_E_ARG, "hier_create: P/R missing");
    for (int l = 0; l < nlevels; ++l) {  // (before anything below dereferences them)
        if (!A[l]) return fail(PAMG_E_ARG, "hier_create: A[%d] is NULL", l);
        if (l < nlevels - 1 && (!P[l] || !R[l])) return fail(PAMG_E_ARG, "hier_create: P/R[%d] is NULL", l);
    }
    const int L = nlevels, nr = ctx->nranks, me = ctx->rank;
    if (nr == 1 || L == 1) rep_level = L - 1;
    if (rep_level < (L > 1 ? 1 : 0) || rep_level > L - 1)
        return fail(PAMG_E_ARG, "hier_create: rep_level %d outside [1, %d]", rep_level, L - 1);
    if (nr > 1 && !rep_offsets)
        return fail(PAMG_E_ARG, "hier_create: rep_offsets required with %d ranks", nr);
    CHECK(set_device(ctx));
    std::unique_ptr<pamg_hier, int (*)(pamg_hier*)> H(new pamg_hier, pamg_hier_destroy);
    H->ctx = ctx;
    ctx_ref(ctx);  // (before the first failure point: the deleter drops it)
    H->L = nlevels;
    H->rep = rep_level;
    // graph replay on one part and on RCCL multi-part runs (RCCL captures its p2p and
    // collectives); never with the host debug transport (host callbacks)
    H->use_graph = nr == 1 || (ctx->comm != nullptr && !ctx->host_fn);
    H->coffs.assign(nr + 1, 0);
    if (rep_offsets) {
        for (int q = 0; q <= nr; ++q) H->coffs[q] = rep_offsets[q];
    } else {
        H->coffs[1] = A[rep_level]->nrows;
    }
    for (int q = 0; q < nr; ++q) {
        if (H->coffs[q + 1] < H->coffs[q]) return fail(PAMG_E_ARG, "hier_create: rep_offsets not monotone");
        H->cmax = std::max(H->cmax, H->coffs[q + 1] - H->coffs[q]);
    }
    const int64_t n_rep = H->coffs[nr], rep_own = H->coffs[me + 1] - H->coffs[me];
    H->A.assign(A, A + L);
    H->P.assign(L, nullptr);
    H->R.assign(L, nullptr);
    H->omega.assign(omega, omega + L);
    H->x.assign(L, nullptr);
    H->b.assign(L, nullptr);
    H->t.assign(L, nullptr);
    H->r.assign(L, nullptr);
    H->nown.assign(L, 0);
    for (int l = 0; l < L; ++l) {
        if (!A[l]) return fail(PAMG_E_ARG, "hier_create: A[%d] is NULL", l);
        // levels >= rep are whole on every rank (the coarsest may be passed distributed: only
        // its inverse is used)
        H->nown[l] = (l == rep_level && L > 1) ? n_rep : A[l]->nrows;
    }
    if (L > 1 && nr > 1 && rep_level < L - 1 && A[rep_level]->nrows != n_rep)
        return fail(PAMG_E_ARG, "hier_create: A[%d] must be whole (%lld rows) on every rank",
                    rep_level, (long long)n_rep);
    for (int l = 0; l < L - 1; ++l) {
        if (!P[l] || !R[l]) return fail(PAMG_E_ARG, "hier_create: P/R[%d] is NULL", l);
        H->P[l] = P[l];
        H->R[l] = R[l];
        if (!A[l]->d_diag && A[l]->nrows > 0)  // (a part may own no row of a coarse level)
            return fail(PAMG_E_SETUP, "hier_create: A[%d] lacks a nonzero diagonal", l);
        const int64_t r_rows = (l + 1 == rep_level) ? rep_own : H->nown[l + 1];
        if (P[l]->nrows != A[l]->nrows || R[l]->nrows != r_rows)
            return fail(PAMG_E_ARG, "hier_create: level %d operator shapes inconsistent", l);
        if (l + 1 >= rep_level && (P[l]->plan || P[l]->ncols != H->nown[l + 1]))
            return fail(PAMG_E_ARG, "hier_create: P[%d] must read the whole level-%d vector (no plan, %lld columns)",
                        l, l + 1, (long long)H->nown[l + 1]);
    }
    // ghost capacity of each level's vectors = max over the plans that read them
    for (int l = 0; l < L; ++l) {
        int64_t g = 0;
        if (A[l]->plan) g = std::max(g, A[l]->plan->n_ghost);
        if (l < L - 1 && R[l]->plan) g = std::max(g, R[l]->plan->n_ghost);
        if (l > 0 && P[l - 1]->plan) g = std::max(g, P[l - 1]->plan->n_ghost);
        const int64_t n = H->nown[l] + g + kVecPad;
        if (l > 0) {
            CHECK(dalloc(&H->x[l], n));
            CHECK(dalloc(&H->b[l], n));
            CHECK(dzero(ctx, H->x[l], sizeof(double) * n));
            CHECK(dzero(ctx, H->b[l], sizeof(double) * n));
        }
        if (l < L - 1) {
            CHECK(dalloc(&H->t[l], n));
            CHECK(dalloc(&H->r[l], n));
            CHECK(dzero(ctx, H->t[l], sizeof(double) * n));
            CHECK(dzero(ctx, H->r[l], sizeof(double) * n));
        }
    }
    // coarsest level
    H->nc = n_coarse;
    if (H->nown[L - 1] != n_coarse && !(L == 1 && nr > 1))
        return fail(PAMG_E_ARG, "hier_create: coarsest level has %lld rows, n_coarse = %lld",
                    (long long)H->nown[L - 1], (long long)n_coarse);
    if (L == 1 && (n_rep != n_coarse || rep_own != A[0]->nrows))
        return fail(PAMG_E_ARG, "hier_create: rep_offsets inconsistent with the one-level hierarchy");
    {
        // row-major on the device: one wave reads a row of A^-1 coalesced (k_dense_gemv)
        std::vector<double> rm((size_t)n_coarse * n_coarse);
        for (int64_t j = 0; j < n_coarse; ++j)
            for (int64_t i = 0; i < n_coarse; ++i) rm[(size_t)i * n_coarse + j] = ainv[(size_t)j * n_coarse + i];
        CHECK(dalloc(&H->d_ainv, n_coarse * n_coarse));
        HIPC(hipMemcpy(H->d_ainv, rm.data(), sizeof(double) * rm.size(), hipMemcpyHostToDevice));
    }
    if (nr > 1) {
        CHECK(dalloc(&H->d_bgather, (int64_t)nr * H->cmax + n_rep + kVecPad));
        CHECK(dalloc(&H->d_bsend, H->cmax + kVecPad));
        CHECK(dzero(ctx, H->d_bsend, sizeof(double) * (H->cmax + kVecPad)));
    }
    H->prof_ms.assign((size_t)L * 6, 0.0);
    *out = H.release();
    return PAMG_OK;
}

static void drop_cycle_graph(pamg_hier* H) {
    if (H->gexec) (void)hipGraphExecDestroy(H->gexec);
    H->gexec = nullptr;
    H->g_x = H->g_b = nullptr;
}

static void drop_pipe_graphs(pamg_hier* H) {
    for (hipGraphExec_t* g : {&H->g_head, &H->g_steady[0], &H->g_steady[1], &H->g_tail[0], &H->g_tail[1]}) {
        if (*g) (void)hipGraphExecDestroy(*g);
        *g = nullptr;
    }
    H->gp_x = H->gp_b = nullptr;
}

// the two half-iteration graphs of pamg_pcg_resident (they hold a whole V-cycle)
static void drop_pcg_graphs(pamg_hier* H) {
    for (hipGraphExec_t& g : H->g_pcg) {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
    }
    H->gr_x = nullptr;
}

// the multi-column cycle's graph (SPEC §S13)
static void drop_multi_graph(pamg_hier* H) {
    if (H->gm_exec) (void)hipGraphExecDestroy(H->gm_exec);
    H->gm_exec = nullptr;
    H->gm_x = H->gm_b = nullptr;
    H->gm_k = 0;
}

static void drop_graph(pamg_hier* H) {
    drop_cycle_graph(H);
    drop_pipe_graphs(H);
    drop_pcg_graphs(H);
    drop_multi_graph(H);
}

// the k-column work vectors of the multi-column calls
static void free_multi(pamg_hier* H) {
    for (std::vector<double*>* set : {&H->mx, &H->mb, &H->mt, &H->mr}) {
        for (double*& p : *set) dfree(p);
        set->clear();
    }
    dfree(H->mu0);
    dfree(H->mpcg_r);
    dfree(H->mpcg_z);
    dfree(H->mpcg_p);
    dfree(H->mpcg_q);
    H->mc_cols = 0;
}

int pamg_hier_destroy(pamg_hier* H) {
    if (!H) return PAMG_OK;
    (void)hipSetDevice(H->ctx->device);
    (void)hipStreamSynchronize(H->ctx->s_comp);
    drop_graph(H);
    for (size_t l = 0; l < H->t.size(); ++l) {
        if (l > 0) {
            dfree(H->x[l]);
            dfree(H->b[l]);
        }
        dfree(H->t[l]);
        dfree(H->r[l]);
    }
    dfree(H->d_ainv);
    dfree(H->d_bgather);
    dfree(H->d_bsend);
    dfree(H->pcg_r);
    dfree(H->pcg_z);
    dfree(H->pcg_p);
    dfree(H->pcg_q);
    dfree(H->pcg_S);
    dfree(H->pcg_hist);
    if (H->pcg_slot) (void)hipHostFree(H->pcg_slot);
    if (H->pcg_stage) (void)hipHostFree(H->pcg_stage);
    for (auto e : H->pcg_ev) (void)hipEventDestroy(e);
    dfree(H->u0);
    free_multi(H);
    dfree(H->d_perm);
    dfree(H->px);
    dfree(H->pb);
    for (auto e : H->ev) (void)hipEventDestroy(e);
    pamg_ctx* owner = H->ctx;
    delete H;
    ctx_unref(owner);
    return PAMG_OK;
}

int pamg_hier_set_graph(pamg_hier* H, int enable) {
    if (!H) return fail(PAMG_E_ARG, "hier_set_graph: NULL");
    if (enable && sync_transport(H->ctx))
        return fail(PAMG_E_STATE, "hier_set_graph: the host debug / in-process transports cannot be graph-captured");
    H->use_graph = enable != 0;
    if (!H->use_graph) drop_graph(H);
    return PAMG_OK;
}

int pamg_hier_set_sweeps(pamg_hier* H, int nu1, int nu2) {
    if (!H || nu1 < 1 || nu2 < 1 || nu1 > 64 || nu2 > 64)
        return fail(PAMG_E_ARG, "hier_set_sweeps: need 1 <= nu1, nu2 <= 64");
    if (H->nu1 != nu1 || H->nu2 != nu2) {
        (void)hipSetDevice(H->ctx->device);
        (void)hipStreamSynchronize(H->ctx->s_comp);
        drop_graph(H);  // the captured cycle has the old sweep counts
    }
    H->nu1 = nu1;
    H->nu2 = nu2;
    return PAMG_OK;
}

int pamg_hier_set_omega(pamg_hier* H, const double* omega) {
    if (!H) return fail(PAMG_E_ARG, "hier_set_omega: NULL");
    const int nl = H->L - 1;
    if (nl > 0 && !omega) return fail(PAMG_E_ARG, "hier_set_omega: omega is NULL");
    bool same = true;
    for (int l = 0; l < nl; ++l) {
        if (!(omega[l] > 0.0) || !std::isfinite(omega[l]))
            return fail(PAMG_E_ARG, "hier_set_omega: omega[%d] must be finite and > 0", l);
        same = same && omega[l] == H->omega[l];
    }
    if (!same) {
        (void)hipSetDevice(H->ctx->device);
        (void)hipStreamSynchronize(H->ctx->s_comp);
        drop_graph(H);  // the captured cycles carry the old weights as launch arguments
    }
    std::copy(omega, omega + nl, H->omega.begin());
    return PAMG_OK;
}

int pamg_hier_set_smoother(pamg_hier* H, int kind, const double* lmax, double ratio) {
    if (!H || kind < PAMG_SMOOTHER_JACOBI || kind > PAMG_SMOOTHER_BLOCK_CHEBYSHEV)
        return fail(PAMG_E_ARG, "hier_set_smoother: bad hierarchy or smoother kind");
    const int nl = H->L - 1;
    const bool is_block = kind == PAMG_SMOOTHER_BLOCK_JACOBI || kind == PAMG_SMOOTHER_BLOCK_CHEBYSHEV;
    const bool is_cheb = kind == PAMG_SMOOTHER_CHEBYSHEV || kind == PAMG_SMOOTHER_BLOCK_CHEBYSHEV;
    if (is_block) {
        bool any = false;
        for (int l = 0; l < nl; ++l) any = any || H->A[l]->bs > 1;
        if (!any)
            return fail(PAMG_E_STATE, "hier_set_smoother: a block smoother needs block data on a level's matrix "
                        "(pamg_mat_set_block_diag)");
    }
    std::vector<double> lm;
    if (is_cheb) {
        if (!(ratio > 1.0) || !std::isfinite(ratio)) return fail(PAMG_E_ARG, "hier_set_smoother: ratio must be > 1");
        if (nl > 0 && !lmax) return fail(PAMG_E_ARG, "hier_set_smoother: lmax is NULL");
        for (int l = 0; l < nl; ++l) {
            if (!(lmax[l] > 0.0) || !std::isfinite(lmax[l]))
                return fail(PAMG_E_ARG, "hier_set_smoother: lmax[%d] must be > 0", l);
            lm.push_back(lmax[l]);
        }
    }
    // (a block smoother always drops: the matrices' block data may have changed since the capture)
    const bool same = !is_block && kind == H->smoother &&
                      (kind == PAMG_SMOOTHER_JACOBI || (lm == H->cheb_lmax && ratio == H->cheb_ratio));
    if (!same) {
        (void)hipSetDevice(H->ctx->device);
        (void)hipStreamSynchronize(H->ctx->s_comp);
        drop_graph(H);  // the captured cycle has the old smoother
    }
    H->smoother = kind;
    H->cheb_lmax.clear();
    H->cheb_c1.clear();
    H->cheb_c2.clear();
    if (is_cheb) {
        H->cheb_ratio = ratio;
        H->cheb_lmax = lm;
        H->cheb_c1.assign(nl, std::vector<double>(kChebMaxDeg));
        H->cheb_c2.assign(nl, std::vector<double>(kChebMaxDeg));
        for (int l = 0; l < nl; ++l) cheb_coeffs(lm[l], ratio, kChebMaxDeg, H->cheb_c1[l].data(), H->cheb_c2[l].data());
    }
    return PAMG_OK;
}

int pamg_chebyshev_coeffs(double lmax, double ratio, int degree, double* c1, double* c2) {
    if (!c1 || !c2 || !(lmax > 0.0) || !(ratio > 1.0) || !std::isfinite(lmax) || !std::isfinite(ratio) || degree < 1 ||
        degree > kChebMaxDeg)
        return fail(PAMG_E_ARG, "chebyshev_coeffs: need lmax > 0, ratio > 1, 1 <= degree <= %d", kChebMaxDeg);
    cheb_coeffs(lmax, ratio, degree, c1, c2);
    return PAMG_OK;
}

int pamg_chebyshev(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* tmp1, pamg_vec* tmp2,
                   double lmax, double ratio, int degree) {
    if (!ctx || !A || !x || !b || !tmp1 || !tmp2) return fail(PAMG_E_ARG, "chebyshev: NULL");
    double c1[kChebMaxDeg], c2[kChebMaxDeg];
    CHECK(pamg_chebyshev_coeffs(lmax, ratio, degree, c1, c2));
    if (A->nrows != (A->plan ? A->plan->n_own : A->ncols) || A->interior.pnc || A->interior.rpat)
        return fail(PAMG_E_ARG, "chebyshev: the operator must be square (%lld rows, %lld own columns)",
                    (long long)A->nrows, (long long)(A->plan ? A->plan->n_own : A->ncols));
    CHECK(check_vec_for(A, x, "chebyshev"));
    CHECK(check_vec_for(A, tmp1, "chebyshev"));
    CHECK(check_vec_for(A, tmp2, "chebyshev"));
    if (!A->d_diag && A->nrows > 0) return fail(PAMG_E_SETUP, "chebyshev: matrix lacks a nonzero diagonal");
    if (b->n_own != A->nrows || tmp1 == x || tmp2 == x || tmp1 == tmp2 || b == x || b == tmp1 || b == tmp2)
        return fail(PAMG_E_ARG, "chebyshev: size mismatch or aliasing");
    CHECK(set_device(ctx));
    double* res = nullptr;
    CHECK(cheb_poly(ctx, A, c1, c2, degree, x->d, b->d, tmp1->d, tmp2->d, &res, false));
    if (res != x->d)
        HIPC(hipMemcpyAsync(x->d, res, sizeof(double) * x->n_own, hipMemcpyDeviceToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_estimate_lmax(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* v, pamg_vec* y, int steps, int all_parts,
                       double* lam) {
    if (!ctx || !A || !v || !y || !lam) return fail(PAMG_E_ARG, "estimate_lmax: NULL");
    if (v == y) return fail(PAMG_E_ARG, "estimate_lmax: v and y must differ");
    if (steps < 1 || steps > 64) return fail(PAMG_E_ARG, "estimate_lmax: need 1 <= steps <= 64");
    if (A->nrows != (A->plan ? A->plan->n_own : A->ncols) || A->interior.pnc || A->interior.rpat)
        return fail(PAMG_E_ARG, "estimate_lmax: the operator must be square (%lld rows, %lld own columns)",
                    (long long)A->nrows, (long long)(A->plan ? A->plan->n_own : A->ncols));
    if (!A->d_diag && A->nrows > 0) return fail(PAMG_E_ARG, "estimate_lmax: matrix lacks a nonzero diagonal");
    CHECK(check_vec_for(A, v, "estimate_lmax"));
    if (y->n_own != A->nrows) return fail(PAMG_E_ARG, "estimate_lmax: output size mismatch");
    CHECK(set_device(ctx));
    for (int k = 0; k < steps; ++k) {
        CHECK(apply(ctx, A, pamg::OP_SPMV, v->d, nullptr, y->d, 0.0));
        double sums[2] = {0.0, 0.0};
        CHECK(lmax_sums(ctx, A->nrows, y->d, A->d_diag, v->d, all_parts != 0, sums));
        if (sums[1] == 0.0 || !std::isfinite(sums[1]))
            return fail(PAMG_E_ARG, "estimate_lmax: step %d: sum (a_ii v_i) v_i = %g (a zero or non-finite iterate)",
                        k + 1, sums[1]);
        lam[k] = sums[0] / sums[1];
    }
    return PAMG_OK;
}

// The argument checks the three block entry points share (those of their scalar forms, then the block data).
static int check_block_op(const pamg_mat* A, const char* what) {
    if (A->nrows != (A->plan ? A->plan->n_own : A->ncols) || A->interior.pnc || A->interior.rpat)
        return fail(PAMG_E_ARG, "%s: the operator must be square (%lld rows, %lld own columns)", what,
                    (long long)A->nrows, (long long)(A->plan ? A->plan->n_own : A->ncols));
    if (A->bs < 2) return fail(PAMG_E_STATE, "%s: the matrix carries no block data (pamg_mat_set_block_diag)", what);
    return PAMG_OK;
}

int pamg_block_jacobi(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* tmp, double omega,
                      int nsweeps) {
    if (!ctx || !A || !x || !b || !tmp || nsweeps < 0) return fail(PAMG_E_ARG, "block_jacobi: bad args");
    CHECK(check_block_op(A, "block_jacobi"));
    CHECK(check_vec_for(A, x, "block_jacobi"));
    CHECK(check_vec_for(A, tmp, "block_jacobi"));
    if (b->n_own != A->nrows || tmp == x || b == x || b == tmp)
        return fail(PAMG_E_ARG, "block_jacobi: size mismatch or aliasing");
    CHECK(set_device(ctx));
    double* cur = x->d;
    double* nxt = tmp->d;
    for (int k = 0; k < nsweeps; ++k) {
        CHECK(smooth_step(ctx, A, true, plan::SMOOTH, cur, b->d, nullptr, nxt, 0.0, omega));
        std::swap(cur, nxt);
    }
    if (cur != x->d)
        HIPC(hipMemcpyAsync(x->d, cur, sizeof(double) * x->n_own, hipMemcpyDeviceToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_block_chebyshev(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* x, const pamg_vec* b, pamg_vec* tmp1,
                         pamg_vec* tmp2, double lmax, double ratio, int degree) {
    if (!ctx || !A || !x || !b || !tmp1 || !tmp2) return fail(PAMG_E_ARG, "block_chebyshev: NULL");
    double c1[kChebMaxDeg], c2[kChebMaxDeg];
    CHECK(pamg_chebyshev_coeffs(lmax, ratio, degree, c1, c2));
    CHECK(check_block_op(A, "block_chebyshev"));
    CHECK(check_vec_for(A, x, "block_chebyshev"));
    CHECK(check_vec_for(A, tmp1, "block_chebyshev"));
    CHECK(check_vec_for(A, tmp2, "block_chebyshev"));
    if (b->n_own != A->nrows || tmp1 == x || tmp2 == x || tmp1 == tmp2 || b == x || b == tmp1 || b == tmp2)
        return fail(PAMG_E_ARG, "block_chebyshev: size mismatch or aliasing");
    CHECK(set_device(ctx));
    double* res = nullptr;
    CHECK(cheb_poly(ctx, A, c1, c2, degree, x->d, b->d, tmp1->d, tmp2->d, &res, true));
    if (res != x->d)
        HIPC(hipMemcpyAsync(x->d, res, sizeof(double) * x->n_own, hipMemcpyDeviceToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_estimate_lmax_block(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* v, pamg_vec* y, int steps, int all_parts,
                             double* lam) {
    if (!ctx || !A || !v || !y || !lam) return fail(PAMG_E_ARG, "estimate_lmax_block: NULL");
    if (v == y) return fail(PAMG_E_ARG, "estimate_lmax_block: v and y must differ");
    if (steps < 1 || steps > 64) return fail(PAMG_E_ARG, "estimate_lmax_block: need 1 <= steps <= 64");
    CHECK(check_block_op(A, "estimate_lmax_block"));
    CHECK(check_vec_for(A, v, "estimate_lmax_block"));
    if (y->n_own != A->nrows) return fail(PAMG_E_ARG, "estimate_lmax_block: output size mismatch");
    CHECK(set_device(ctx));
    for (int k = 0; k < steps; ++k) {
        CHECK(apply(ctx, A, pamg::OP_SPMV, v->d, nullptr, y->d, 0.0));
        double sums[2] = {0.0, 0.0};
        CHECK(lmax_sums(ctx, A->nrows, y->d, nullptr, v->d, all_parts != 0, sums, A));
        if (sums[1] == 0.0 || !std::isfinite(sums[1]))
            return fail(PAMG_E_ARG, "estimate_lmax_block: step %d: sum (D_b v)_i v_i = %g (a zero or non-finite iterate)",
                        k + 1, sums[1]);
        lam[k] = sums[0] / sums[1];
    }
    return PAMG_OK;
}

int pamg_hier_set_perm(pamg_hier* H, int64_t n, const int64_t* perm) {
    if (!H) return fail(PAMG_E_ARG, "hier_set_perm: NULL");
    pamg_ctx* ctx = H->ctx;
    CHECK(set_device(ctx));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    dfree(H->d_perm);
    dfree(H->px);
    dfree(H->pb);
    if (!perm || n == 0) return PAMG_OK;
    if (ctx->nranks > 1) return fail(PAMG_E_STATE, "hier_set_perm: one part only (permute a partition's rows before setup)");
    if (H->outer) return fail(PAMG_E_STATE, "hier_set_perm: the hierarchy has an outer operator (pamg_hier_set_outer)");
    const pamg_mat* A0 = H->A[0];
    if (n != H->nown[0] || n != A0->ncols)
        return fail(PAMG_E_ARG, "hier_set_perm: %lld entries for a %lld-row level 0", (long long)n, (long long)H->nown[0]);
    std::vector<int> p(n);
    std::vector<char> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (perm[i] < 0 || perm[i] >= n || seen[perm[i]]) return fail(PAMG_E_ARG, "hier_set_perm: not a permutation");
        seen[perm[i]] = 1;
        p[i] = (int)perm[i];
    }
    CHECK(dalloc(&H->d_perm, n));
    CHECK(dalloc(&H->px, n + kVecPad));
    CHECK(dalloc(&H->pb, n + kVecPad));
    HIPC(hipMemcpy(H->d_perm, p.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    CHECK(dzero(H->ctx, H->px, sizeof(double) * (n + kVecPad)));
    CHECK(dzero(H->ctx, H->pb, sizeof(double) * (n + kVecPad)));
    return PAMG_OK;
}

// SPEC §S15: the operator pamg_pcg, pamg_pcg_resident and pamg_pcg_multi use for b - A x and A p (the exact
// A beside a hierarchy of rounded operators); NULL: A[0] again. The V-cycle is untouched.
int pamg_hier_set_outer(pamg_hier* H, const pamg_mat* A) {
    if (!H) return fail(PAMG_E_ARG, "hier_set_outer: NULL");
    if (A) {
        const pamg_mat* A0 = H->A[0];
        if (H->d_perm) return fail(PAMG_E_STATE, "hier_set_outer: the hierarchy has a level-0 permutation");
        if (A->ctx != H->ctx || A->permuted) return fail(PAMG_E_ARG, "hier_set_outer: an operator of another context or numbering");
        if (A->nrows != A0->nrows || A->ncols != A0->ncols)
            return fail(PAMG_E_ARG, "hier_set_outer: a %lld x %lld operator for a %lld x %lld level 0", (long long)A->nrows,
                        (long long)A->ncols, (long long)A0->nrows, (long long)A0->ncols);
        if (A->plan != A0->plan) return fail(PAMG_E_ARG, "hier_set_outer: the operator has another column plan than level 0");
    }
    CHECK(set_device(H->ctx));
    HIPC(hipStreamSynchronize(H->ctx->s_comp));
    drop_pcg_graphs(H);  // (they hold the q = A p launch)
    H->outer = A;
    return PAMG_OK;
}

int pamg_hier_graph_state(const pamg_hier* H, int* enabled, int* captured, int* failed) {
    if (!H) return fail(PAMG_E_ARG, "hier_graph_state: NULL");
    if (enabled) *enabled = H->use_graph ? 1 : 0;
    if (captured) *captured = (H->gexec || H->g_head) ? 1 : 0;
    if (failed) *failed = H->graph_failed ? 1 : 0;
    return PAMG_OK;
}

int pamg_hier_profile(pamg_hier* H, int enable) {
    if (!H) return fail(PAMG_E_ARG, "hier_profile: NULL");
    H->prof = enable != 0;
    return PAMG_OK;
}

int pamg_hier_profile_read(pamg_hier* H, double* out) {
    if (!H || !out) return fail(PAMG_E_ARG, "hier_profile_read: bad args");
    CHECK(set_device(H->ctx));
    HIPC(hipStreamSynchronize(H->ctx->s_comp));
    for (size_t k = 0; k < H->ev_tag.size(); ++k) {
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, H->ev[2 * k], H->ev[2 * k + 1]));
        H->prof_ms[(size_t)H->ev_tag[k].first * 6 + H->ev_tag[k].second] += ms;
    }
    for (auto e : H->ev) (void)hipEventDestroy(e);
    H->ev.clear();
    H->ev_tag.clear();
    std::copy(H->prof_ms.begin(), H->prof_ms.end(), out);
    std::fill(H->prof_ms.begin(), H->prof_ms.end(), 0.0);
    return PAMG_OK;
}

// ncycles V-cycles on raw device vectors (graph replay when enabled; the captured graph is
// keyed on the vector addresses and the zero-guess flag).
// The k_sym_chain launch of a steady segment: the previous cycle's level-0 post-smoothing
// (t_prev -> x), this cycle's pre-smoothing (x -> t_next) and residual (t_next -> r[0]).
static int launch_chain3(pamg_hier* H, double* x, const double* b, const double* t_prev, double* t_next) {
    const pamg_mat* A = H->A[0];
    if (A->sym.tb_part) {  // one part of several: the blocked pass on the slab's inner planes
        double* out[3] = {x, t_next, H->r[0]};
        return sweeps_part(H->ctx, A, 3, t_prev, out, b, H->omega[0]);
    }
    pamg::TbArgs ta;
    ta.nstages = 3;
    ta.last_resid = true;
    ta.in0 = t_prev;
    // the post-smoothed iterate of cycle k is read only by this launch's next stage (from LDS):
    // the V-cycle's x is written by the tail's post-smoothing, so a steady chain stores it only
    // when asked (Options::chain_store_x; same bits either way)
    ta.out[0] = pamg::options().chain_store_x ? x : nullptr;
    ta.out[1] = t_next;
    ta.out[2] = H->r[0];
    ta.b = b;
    ta.omega = H->omega[0];
    pamg::launch_sym_tb(*A, ta, H->ctx->s_comp);
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// Segments of the cross-cycle pipeline. seg 0: head (first cycle, no level-0 post-smoothing,
// iterate in t[0]); 1 / 2: steady, the iterate moving t[0] -> u0 / u0 -> t[0]; 3 / 4: tail (the
// last post-smoothing from t[0] / u0).
static int pipe_enqueue(pamg_hier* H, double* x, const double* b, int seg) {
    L0Seg sg;
    sg.post = false;
    if (seg == 0) return vcycle_enqueue(H, x, b, false, sg);
    double* t0 = H->t[0];
    double* u0 = H->u0;
    if (seg == 1 || seg == 2) {
        double* prev = seg == 1 ? t0 : u0;
        double* next = seg == 1 ? u0 : t0;
        {
            ProfScope p(H, 0, 0, H->ctx->s_comp);
            CHECK(launch_chain3(H, x, b, prev, next));
        }
        sg.given = true;
        sg.t0 = seg == 1 ? plan::U0 : plan::T;
        return vcycle_enqueue(H, x, b, false, sg);
    }
    ProfScope p(H, 0, 4, H->ctx->s_comp);
    return apply(H->ctx, H->A[0], pamg::OP_JACOBI, seg == 3 ? t0 : u0, b, x, H->omega[0]);
}

// Eligible for the cross-cycle pipeline: one part, V(1, 1), level 0 in the symmetric layout with
// chain schedules, fusion on, a stationary run of >= 2 cycles from a given guess.
// Invariant across ranks: the decision is per rank (A->sym.tb_part depends on the
// part's shape), so ranks may disagree — one pipelining, its neighbour running separate cycles.
// That is correct only because both schedules issue the same exchanges in the same order on
// every level: pre-smoothing (A), residual (A), restriction (R), [tail all-gather], prolongation
// (P), post-smoothing (A) — the pipeline's chain does post-smoothing(k) (A), pre-smoothing(k+1)
// (A), residual(k+1) (A) through sweeps_part, one exchange per stage, in cycle order. Any change
// to either schedule must keep that sequence (tests/test_gpu_multipart.py: mixed ranks).
static bool pipe_ok(const pamg_hier* H, int ncycles, bool zero0) {
    if (zero0 || ncycles < 2 || H->L < 2 || H->prof || !pamg::options().jr_fuse || H->nu1 != 1 || H->nu2 != 1)
        return false;
    if (H->smoother != PAMG_SMOOTHER_JACOBI) return false;  // (the chain kernels are Jacobi sweeps)
    const pamg_mat* A = H->A[0];
    if (!A->interior.sym) return false;
    return (H->ctx->nranks == 1 && A->sym.tb_ok && !(A->plan && !A->plan->nbr.empty())) || A->sym.tb_part;
}

// the spare level-0 vector (the pipeline's second iterate; the Chebyshev cycle's fourth ring vector)
static int ensure_u0(pamg_hier* H) {
    if (H->u0) return PAMG_OK;
    const int64_t n = H->nown[0] + (H->A[0]->plan ? H->A[0]->plan->n_ghost : 0) + kVecPad;
    CHECK(dalloc(&H->u0, n));
    CHECK(dzero(H->ctx, H->u0, sizeof(double) * n));
    return PAMG_OK;
}

static int vcycle_pipe(pamg_hier* H, double* x, const double* b, int ncycles) {
    pamg_ctx* ctx = H->ctx;
    CHECK(ensure_u0(H));
    const int K = ncycles;
    auto seg_of = [K](int k) { return k == 0 ? 0 : k < K ? (k % 2 == 1 ? 1 : 2) : ((K - 1) % 2 == 1 ? 4 : 3); };
    if (H->use_graph && (!H->g_head || H->gp_x != x || H->gp_b != b)) {
        drop_pipe_graphs(H);
        bool ok = true;
        hipGraphExec_t* slot[5] = {&H->g_head, &H->g_steady[0], &H->g_steady[1], &H->g_tail[0], &H->g_tail[1]};
        for (int sgi = 0; sgi < 5 && ok; ++sgi)
            ok = capture_graph(ctx->s_comp, [&] { return pipe_enqueue(H, x, b, sgi); }, slot[sgi]);
        if (ok) {
            H->gp_x = x;
            H->gp_b = b;
        } else {
            capture_failed(H, "pipelined V-cycle");
            drop_pipe_graphs(H);
        }
    }
    for (int k = 0; k <= K; ++k) {
        const int sg = seg_of(k);
        if (H->use_graph && H->g_head) {
            hipGraphExec_t ge = sg == 0 ? H->g_head : sg <= 2 ? H->g_steady[sg - 1] : H->g_tail[sg - 3];
            HIPC(hipGraphLaunch(ge, ctx->s_comp));
        } else {
            CHECK(pipe_enqueue(H, x, b, sg));
        }
    }
    return PAMG_OK;
}

static int vcycle_raw(pamg_hier* H, double* x, const double* b, int ncycles, bool zero0) {
    pamg_ctx* ctx = H->ctx;
    if (zero0 && ncycles != 1) return fail(PAMG_E_ARG, "vcycle: zero initial guess applies to one cycle");
    // stationary runs of >= 2 cycles: the cross-cycle pipeline (same operations, same bits)
    if (pipe_ok(H, ncycles, zero0)) return vcycle_pipe(H, x, b, ncycles);
    // the spare level-0 vector where the plan names it, allocated before any capture
    if (H->L > 1 && !H->u0 && plan::plan_cycle(cycle_spec(H, zero0)).needs_u0) CHECK(ensure_u0(H));
    if (H->use_graph && !H->prof && (!H->gexec || H->g_x != x || H->g_b != b || H->g_zero0 != zero0)) {
        // Capture one cycle (RCCL exchanges included on several parts: RCCL records its
        // send/recv/all-gather as graph nodes). If capture fails, fall back to eager launches
        // for this hierarchy: both paths issue the same RCCL sequence, so ranks that did
        // capture and ranks that did not still match.
        drop_cycle_graph(H);
        if (capture_graph(ctx->s_comp, [&] { return vcycle_enqueue(H, x, b, zero0); }, &H->gexec)) {
            H->g_x = x;
            H->g_b = b;
            H->g_zero0 = zero0;
        } else {
            H->gexec = nullptr;
            capture_failed(H, "V-cycle");
        }
    }
    if (H->use_graph && !H->prof && H->gexec) {
        for (int k = 0; k < ncycles; ++k) HIPC(hipGraphLaunch(H->gexec, ctx->s_comp));
    } else {
        for (int k = 0; k < ncycles; ++k) CHECK(vcycle_enqueue(H, x, b, zero0 && k == 0));
    }
    return PAMG_OK;
}

// The caller's level-0 vectors in the device numbering: with a level-0 permutation, b is
// gathered into pb and (unless the guess is zero) x into px; without one they are used as is.
struct DeviceSpace {
    pamg_hier* H;
    double* x;
    const double* b;
    DeviceSpace(pamg_hier* h, pamg_vec* xv, const pamg_vec* bv, bool gather_x) : H(h), x(xv->d), b(bv->d) {
        if (!H->d_perm) return;
        const int64_t n = H->nown[0];
        hipStream_t s = H->ctx->s_comp;
        pamg::launch_permute(n, H->d_perm, bv->d, H->pb, false, s);
        if (gather_x) pamg::launch_permute(n, H->d_perm, xv->d, H->px, false, s);
        x = H->px;
        b = H->pb;
    }
    // x back to the caller's numbering
    void finish(pamg_vec* xv) {
        if (H->d_perm) pamg::launch_permute(H->nown[0], H->d_perm, H->px, xv->d, true, H->ctx->s_comp);
    }
};

static int vcycle_common(pamg_ctx* ctx, pamg_hier* H, pamg_vec* x, const pamg_vec* b, int ncycles) {
    if (!ctx || !H || !x || !b || ncycles < 0 || H->ctx != ctx) return fail(PAMG_E_ARG, "vcycle: bad args");
    const pamg_mat* A0 = H->A[0];
    CHECK(check_vec_for(A0, x, "vcycle"));
    if (b->n_own != A0->nrows) return fail(PAMG_E_ARG, "vcycle: b size mismatch");
    CHECK(set_device(ctx));
    DeviceSpace d(H, x, b, true);
    CHECK(vcycle_raw(H, d.x, d.b, ncycles, false));
    d.finish(x);
    HIPC(hipGetLastError());
    return PAMG_OK;
}

int pamg_vcycle_async(pamg_ctx* ctx, pamg_hier* H, pamg_vec* x, const pamg_vec* b, int ncycles) {
    return vcycle_common(ctx, H, x, b, ncycles);
}

int pamg_vcycle(pamg_ctx* ctx, pamg_hier* H, pamg_vec* x, const pamg_vec* b, int ncycles,
                double* res_hist) {
    if (!res_hist) {
        CHECK(vcycle_common(ctx, H, x, b, ncycles));
        HIPC(hipStreamSynchronize(ctx->s_comp));
        return PAMG_OK;
    }
    if (!ctx || !H || !x || !b || ncycles < 0 || H->ctx != ctx) return fail(PAMG_E_ARG, "vcycle: bad args");
    if (H->L < 1 || (!H->t[0] && H->L > 1)) return fail(PAMG_E_ARG, "vcycle: bad hierarchy");
    CHECK(check_vec_for(H->A[0], x, "vcycle"));
    if (b->n_own != H->A[0]->nrows) return fail(PAMG_E_ARG, "vcycle: b size mismatch");
    CHECK(set_device(ctx));
    DeviceSpace d(H, x, b, true);
    for (int k = 0; k < ncycles; ++k) {
        CHECK(vcycle_raw(H, d.x, d.b, 1, false));
        // r = b - A x into the level-0 residual buffer (1-level hierarchies use a temporary)
        double* r = H->L > 1 ? H->r[0] : nullptr;
        double* tmp = nullptr;
        if (!r) {
            CHECK(dalloc(&tmp, H->nown[0] + kVecPad));
            r = tmp;
        }
        int rc = apply(ctx, H->A[0], pamg::OP_RESID, d.x, d.b, r, 0.0);
        double s = 0.0;
        if (rc == PAMG_OK) rc = reduce_scalar(ctx, H->nown[0], r, r, &s);
        dfree(tmp);
        CHECK(rc);
        res_hist[k] = std::sqrt(s);
    }
    d.finish(x);
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

// Preconditioned CG with one V-cycle from a zero guess as M^-1 (SPEC §S8). The V(1,1) cycle
// with R = P^T and the same weighted Jacobi before and after is symmetric, so CG applies.
int pamg_pcg(pamg_ctx* ctx, pamg_hier* H, pamg_vec* x, const pamg_vec* b, double rtol,
             int maxit, int* iters, double* res_hist) {
    if (!ctx || !H || !x || !b || maxit < 0 || !(rtol >= 0.0) || H->ctx != ctx)
        return fail(PAMG_E_ARG, "pcg: bad args");
    const pamg_mat* A = H->outer ? H->outer : H->A[0];
    CHECK(check_vec_for(A, x, "pcg"));
    if (b->n_own != A->nrows) return fail(PAMG_E_ARG, "pcg: b size mismatch");
    CHECK(set_device(ctx));
    const int64_t n = A->nrows;
    int64_t g = A->plan ? A->plan->n_ghost : 0;
    if (H->L > 1 && H->R[0]->plan) g = std::max(g, H->R[0]->plan->n_ghost);
    const int64_t cap = n + g + kVecPad;
    if (!H->pcg_r) {
        CHECK(dalloc(&H->pcg_r, cap));
        CHECK(dalloc(&H->pcg_z, cap));
        CHECK(dalloc(&H->pcg_p, cap));
        CHECK(dalloc(&H->pcg_q, cap));
        for (double* p : {H->pcg_r, H->pcg_z, H->pcg_p, H->pcg_q})
            CHECK(dzero(ctx, p, sizeof(double) * cap));
    }
    hipStream_t s = ctx->s_comp;
    double *r = H->pcg_r, *z = H->pcg_z, *p = H->pcg_p, *q = H->pcg_q;
    // with a level-0 permutation the whole iteration runs in the device numbering
    DeviceSpace d(H, x, b, true);
    double* xd = d.x;
    CHECK(apply(ctx, A, pamg::OP_RESID, xd, d.b, r, 0.0));
    double rr = 0.0;
    CHECK(reduce_scalar(ctx, n, r, r, &rr));
    const double nr0 = std::sqrt(rr);
    if (res_hist) res_hist[0] = nr0;
    int k = 0;
    if (nr0 > 0.0 && maxit > 0) {
        CHECK(vcycle_raw(H, z, r, 1, true));
        HIPC(hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        double rz = 0.0;
        CHECK(reduce_scalar(ctx, n, r, z, &rz));
        while (k < maxit) {
            ++k;
            CHECK(apply(ctx, A, pamg::OP_SPMV, p, nullptr, q, 0.0));
            double pq = 0.0;
            CHECK(reduce_scalar(ctx, n, p, q, &pq));
            const double alpha = rz / pq;
            // x += alpha p; r -= alpha q; rr = r.r in one pass (bits of the unfused sequence)
            CHECK(reduce_with(ctx, n, &rr, [&](int np, double* parts, double* res, hipStream_t st) {
                pamg::launch_cg_update(n, alpha, p, q, xd, r, parts, np, res, st);
            }));
            const double nr = std::sqrt(rr);
            if (res_hist) res_hist[k] = nr;
            if (nr <= rtol * nr0) break;
            CHECK(vcycle_raw(H, z, r, 1, true));
            double rz_new = 0.0;
            CHECK(reduce_scalar(ctx, n, r, z, &rz_new));
            const double beta = rz_new / rz;
            rz = rz_new;
            pamg::launch_axpby(n, 1.0, z, beta, p, s);
        }
    }
    d.finish(x);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (iters) *iters = k;
    return PAMG_OK;
}

// SPEC §S11: the largest double c with RN(sqrt(c)) <= thr, so that rr <= c is the test
// RN(sqrt(rr)) <= thr (RN o sqrt is monotone). Host arithmetic only.
int pamg_pcg_rr_threshold(double thr, double* out) {
    if (!out || !(thr >= 0.0)) return fail(PAMG_E_ARG, "pcg_rr_threshold: need thr >= 0 and an output");
    const double inf = std::numeric_limits<double>::infinity();
    if (thr == 0.0 || thr == inf) {
        *out = thr;
        return PAMG_OK;
    }
    double c = thr * thr;  // within a rounding of the answer, save where it underflows or overflows
    int steps = 0;
    for (double up = std::nextafter(c, inf); std::sqrt(up) <= thr; up = std::nextafter(c, inf)) {
        c = up;
        if (++steps > 4) return fail(PAMG_E_STATE, "pcg_rr_threshold: more than 4 steps up from thr^2 (thr = %a)", thr);
    }
    while (std::sqrt(c) > thr) {
        c = std::nextafter(c, -inf);
        if (++steps > 4) return fail(PAMG_E_STATE, "pcg_rr_threshold: more than 4 steps down from thr^2 (thr = %a)", thr);
    }
    *out = c;
    return PAMG_OK;
}

}  // extern "C"

namespace {

// One half of a §S11 iteration on the compute stream. Half 0: q = A p, (p, q), alpha, the x / r
// update, r.r, the check, and {k, done} to the pinned slot. Half 1: z = M^-1 r, (r, z), beta,
// p = z + beta p.
int pcg_half_enqueue(pamg_hier* H, double* xd, int half) {
    pamg_ctx* ctx = H->ctx;
    hipStream_t s = ctx->s_comp;
    const int64_t n = H->A[0]->nrows;
    const int np = pamg::dot_partials(n);
    double *r = H->pcg_r, *z = H->pcg_z, *p = H->pcg_p, *q = H->pcg_q;
    if (half == 0) {
        CHECK(apply(ctx, H->outer ? H->outer : H->A[0], pamg::OP_SPMV, p, nullptr, q, 0.0));
        pamg::launch_pcg_half_a(n, H->pcg_S, p, q, xd, r, ctx->d_red, np, H->pcg_hist, s);
        HIPC(hipMemcpyAsync(H->pcg_slot, &H->pcg_S->k, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    } else {
        CHECK(vcycle_enqueue(H, z, r, true));
        pamg::launch_pcg_half_b(n, H->pcg_S, r, z, p, ctx->d_red, np, s);
    }
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// Capture the two halves for this device x (once per (H, x), like vcycle_raw's cycle graph); on
// failure the hierarchy goes to eager launches of the same kernels.
void pcg_capture(pamg_hier* H, double* xd) {
    pamg_ctx* ctx = H->ctx;
    drop_pcg_graphs(H);
    bool ok = true;
    for (int half = 0; half < 2 && ok; ++half)
        ok = capture_graph(ctx->s_comp, [&] { return pcg_half_enqueue(H, xd, half); }, &H->g_pcg[half]);
    if (ok) {
        H->gr_x = xd;
        return;
    }
    capture_failed(H, "PCG iteration");
    drop_pcg_graphs(H);
}

}  // namespace

extern "C" {

// Preconditioned CG as pamg_pcg, with alpha, beta, rho and r.r in device memory and the iteration
// replayed as two graphs (SPEC §S11): the host waits for rr_0, then once per iteration
// (lookahead 0) or only for the outcome of iteration j - lookahead (lookahead >= 1).
int pamg_pcg_resident(pamg_ctx* ctx, pamg_hier* H, pamg_vec* x, const pamg_vec* b, double rtol, int maxit,
                      int lookahead, int* iters, double* res_hist, int stats[2]) {
    if (!ctx || !H || !x || !b || maxit < 0 || !(rtol >= 0.0) || lookahead < 0 || H->ctx != ctx)
        return fail(PAMG_E_ARG, "pcg_resident: bad args");
    if (ctx->nranks > 1)
        return fail(PAMG_E_STATE, "pcg_resident: one part only (the scalars are not summed across ranks; use pamg_pcg)");
    const pamg_mat* A = H->outer ? H->outer : H->A[0];
    CHECK(check_vec_for(A, x, "pcg_resident"));
    if (b->n_own != A->nrows) return fail(PAMG_E_ARG, "pcg_resident: b size mismatch");
    CHECK(set_device(ctx));
    const int64_t n = A->nrows;
    int64_t g = A->plan ? A->plan->n_ghost : 0;
    if (H->L > 1 && H->R[0]->plan) g = std::max(g, H->R[0]->plan->n_ghost);
    const int64_t cap = n + g + kVecPad;
    if (!H->pcg_r) {
        CHECK(dalloc(&H->pcg_r, cap));
        CHECK(dalloc(&H->pcg_z, cap));
        CHECK(dalloc(&H->pcg_p, cap));
        CHECK(dalloc(&H->pcg_q, cap));
        for (double* p : {H->pcg_r, H->pcg_z, H->pcg_p, H->pcg_q})
            CHECK(dzero(ctx, p, sizeof(double) * cap));
    }
    hipStream_t s = ctx->s_comp;
    if (!H->pcg_S) {
        CHECK(dalloc(&H->pcg_S, 1));
        CHECK(dzero(ctx, H->pcg_S, sizeof(pamg::PcgScalars)));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&H->pcg_slot), 2 * sizeof(int)));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&H->pcg_stage), 4 * sizeof(double)));
    }
    if (H->pcg_hist_cap < (int64_t)maxit + 1) {
        HIPC(hipStreamSynchronize(s));
        drop_pcg_graphs(H);  // they carry the history's address
        dfree(H->pcg_hist);
        H->pcg_hist_cap = 0;
        CHECK(dalloc(&H->pcg_hist, (int64_t)maxit + 1));
        CHECK(dzero(ctx, H->pcg_hist, sizeof(double) * ((size_t)maxit + 1)));
        H->pcg_hist_cap = (int64_t)maxit + 1;
    }
    while ((int)H->pcg_ev.size() < lookahead + 1) {
        hipEvent_t e = nullptr;
        HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        H->pcg_ev.push_back(e);
    }
    double *r = H->pcg_r, *z = H->pcg_z, *p = H->pcg_p;
    DeviceSpace d(H, x, b, true);
    double* xd = d.x;
    CHECK(apply(ctx, A, pamg::OP_RESID, xd, d.b, r, 0.0));
    double rr0 = 0.0;
    CHECK(reduce_scalar(ctx, n, r, r, &rr0));  // the one wait of the prologue
    const double nr0 = std::sqrt(rr0);
    int k = 0, enq = 0;
    if (nr0 > 0.0 && maxit > 0) {
        // the §S8 test RN(sqrt(rr_k)) <= RN(rtol nr0) as a comparison of rr_k itself
        double rr_max = 0.0;
        CHECK(pamg_pcg_rr_threshold(rtol * nr0, &rr_max));
        static_assert(offsetof(pamg::PcgScalars, k) == offsetof(pamg::PcgScalars, rr_max) + sizeof(double) &&
                          offsetof(pamg::PcgScalars, done) == offsetof(pamg::PcgScalars, k) + sizeof(int),
                      "rr_max, k, done are uploaded as one 16-byte piece");
        H->pcg_stage[0] = rr_max;
        const int kd[2] = {0, 0};
        std::memcpy(&H->pcg_stage[1], kd, sizeof(kd));
        H->pcg_stage[2] = rr0;
        H->pcg_slot[0] = H->pcg_slot[1] = 0;
        HIPC(hipMemcpyAsync(&H->pcg_S->rr_max, H->pcg_stage, 2 * sizeof(double), hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(H->pcg_hist, &H->pcg_stage[2], sizeof(double), hipMemcpyHostToDevice, s));
        // the first V-cycle goes through vcycle_raw, which allocates whatever the cycle needs (the
        // Chebyshev rings' spare vector) outside any capture; the captured second halves run the
        // same zero-guess cycle on the same vectors
        CHECK(vcycle_raw(H, z, r, 1, true));
        HIPC(hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        const int np = pamg::dot_partials(n);
        if (np + 1 > ctx->red_cap) return fail(PAMG_E_STATE, "reduction workspace too small");
        pamg::launch_dot(n, r, z, ctx->d_red, np, &H->pcg_S->rz, s);
        HIPC(hipGetLastError());
        if (H->use_graph && !H->prof && (!H->g_pcg[0] || H->gr_x != xd)) pcg_capture(H, xd);
        const bool replay = H->use_graph && !H->prof && H->g_pcg[0] && H->g_pcg[1];
        auto half = [&](int h) -> int {
            if (replay) HIPC(hipGraphLaunch(H->g_pcg[h], s));
            else CHECK(pcg_half_enqueue(H, xd, h));
            return PAMG_OK;
        };
        const int ring = lookahead + 1;
        volatile const int* slot = H->pcg_slot;
        for (int j = 1; j <= maxit; ++j) {
            CHECK(half(0));
            ++enq;
            HIPC(hipEventRecord(H->pcg_ev[j % ring], s));
            if (lookahead == 0) {
                // the outcome of this iteration decides whether its second half is enqueued at all
                HIPC(hipEventSynchronize(H->pcg_ev[j % ring]));
                if (slot[1]) break;
                CHECK(half(1));
                continue;
            }
            CHECK(half(1));
            if (j > lookahead) {
                // the slot holds iteration j - lookahead's outcome or a later one (done never
                // clears): at most `lookahead` iterations were enqueued past convergence
                HIPC(hipEventSynchronize(H->pcg_ev[(j - lookahead) % ring]));
                if (slot[1]) break;
            }
        }
    }
    d.finish(x);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (enq > 0) {
        HIPC(hipMemcpy(&k, &H->pcg_S->k, sizeof(int), hipMemcpyDeviceToHost));
        if (k < 0 || k > enq) return fail(PAMG_E_STATE, "pcg_resident: iteration counter %d of %d enqueued", k, enq);
    }
    if (res_hist) {
        res_hist[0] = nr0;
        if (k > 0) {
            HIPC(hipMemcpy(res_hist + 1, H->pcg_hist + 1, sizeof(double) * k, hipMemcpyDeviceToHost));
            for (int i = 1; i <= k; ++i) res_hist[i] = std::sqrt(res_hist[i]);
        }
    }
    if (iters) *iters = k;
    if (stats) {
        stats[0] = enq;
        stats[1] = enq - k;
    }
    return PAMG_OK;
}

}  // extern "C"

namespace {
// The option keys of pamg_set_option / pamg_get_option: the Options member (pamg_device.h
// documents each) and the values accepted, lo <= value <= hi, powers of two only where pow2.
struct OptionRow {
    const char* key;
    int pamg::Options::*member;
    int64_t lo, hi;
    bool pow2;
};
using O = pamg::Options;
const OptionRow kOptionTable[] = {
    {"tile_nnz", &O::tile_nnz, 1024, 4096, true},
    {"tile_order", &O::tile_order, 0, 1, false},  // 0 natural, 1 banded XCD-blocked
    {"poison_ghosts", &O::poison_ghosts, 0, 1, false},
    {"col24", &O::col24, 0, 1, false},
    {"long_tiles", &O::long_tiles, 0, 1, false},
    {"row_len8", &O::row_len8, 0, 1, false},
    {"value_dict", &O::value_dict, 0, 2, false},
    {"col_dict", &O::col_dict, 0, 1, false},
    {"tile_major", &O::tile_major, 0, 2, false},
    {"col_dict_anchor", &O::col_dict_anchor, 0, 1, false},
    {"col_dict_tile", &O::col_dict_tile, 0, 1, false},
    {"x_stage", &O::x_stage, 0, 1, false},
    {"band_pct", &O::band_pct, 1, 10000, false},
    {"band_pct_restrict", &O::band_pct_restrict, 1, 10000, false},
    {"long_tiles_min", &O::long_tiles_min, 1, 255, false},
    {"tm_tile_dicts", &O::tm_tile_dicts, 0, 1, false},
    {"sym_dia", &O::sym_dia, 0, 1, false},
    {"sym_rows", &O::sym_rows, 1, 2, false},
    {"jr_fuse", &O::jr_fuse, 0, 1, false},
    {"sym_vd", &O::sym_vd, 0, 1, false},
    {"symd_chunks", &O::symd_chunks, 1, 4, true},
    {"sym_zm", &O::sym_zm, 0, 1, false},
    {"tb_xfast", &O::tb_xfast, 0, 1, false},
    {"ell", &O::ell, 0, 1, false},
    {"ell_restrict", &O::ell_restrict, 0, 1, false},
    {"pnc", &O::pnc, 0, 3, false},
    {"rpat", &O::rpat, 0, 1, false},
    {"pnc_compact", &O::pnc_compact, 0, 1, false},
    {"ell_pair", &O::ell_pair, 0, 1, false},
    {"ell_xwin", &O::ell_xwin, 0, 4, false},  // 1 with row classes where they pay, 2 without; 3, 4: as 1, 2 without group pairs
    {"ell_xwin_max", &O::ell_xwin_max, 2, pamg::kEllWinCap, false},
    {"ell_yblock", &O::ell_yblock, 0, 65536, false},
    {"ell_min_rows", &O::ell_min_rows, 0, INT32_MAX, false},
    {"zm_chunks", &O::zm_chunks, 0, 4096, false},
    {"chain_store_x", &O::chain_store_x, 0, 1, false},
};

const OptionRow* find_option(const char* key) {
    for (const OptionRow& r : kOptionTable)
        if (std::strcmp(r.key, key) == 0) return &r;
    return nullptr;
}
}  // namespace

extern "C" {

int pamg_set_option(const char* key, int64_t value) {
    if (!key) return fail(PAMG_E_ARG, "set_option: NULL key");
    const OptionRow* r = find_option(key);
    if (!r || value < r->lo || value > r->hi || (r->pow2 && (value & (value - 1)) != 0))
        return fail(PAMG_E_ARG, "set_option: unknown key or bad value: %s=%lld", key, (long long)value);
    pamg::options().*(r->member) = (int)value;
    return PAMG_OK;
}

int pamg_get_option(const char* key, int64_t* value) {
    if (!key || !value) return fail(PAMG_E_ARG, "get_option: bad args");
    const OptionRow* r = find_option(key);
    if (!r) return fail(PAMG_E_ARG, "get_option: unknown key %s", key);
    *value = pamg::options().*(r->member);
    return PAMG_OK;
}

int pamg_hier_bench_chain(pamg_hier* H, pamg_vec* x, const pamg_vec* b, int reps, double* avg_ms) {
    if (!H || !x || !b || reps < 1 || !avg_ms) return fail(PAMG_E_ARG, "hier_bench_chain: bad args");
    if (!pipe_ok(H, 2, false)) return fail(PAMG_E_STATE, "hier_bench_chain: the hierarchy does not run the cross-cycle pipeline");
    pamg_ctx* ctx = H->ctx;
    CHECK(check_vec_for(H->A[0], x, "hier_bench_chain"));
    CHECK(set_device(ctx));
    CHECK(ensure_u0(H));
    // the warm-up call and the even timed ones t[0] -> u0, the odd ones u0 -> t[0]
    int k = -1;  // (the warm-up call)
    return time_reps(ctx->s_comp, reps, avg_ms, [&]() {
        const bool back = k > 0 && (k & 1);
        ++k;
        return launch_chain3(H, x->d, b->d, back ? H->u0 : H->t[0], back ? H->t[0] : H->u0);
    });
}

int pamg_bench_rowop(pamg_ctx* ctx, const pamg_mat* A, int op, pamg_vec* x, const pamg_vec* b,
                     pamg_vec* y, double omega, int reps, double* avg_ms) {
    if (!ctx || !A || !x || !y || reps < 1 || !avg_ms || op < 0 || op > 6)
        return fail(PAMG_E_ARG, "bench_rowop: bad args");
    if ((op == pamg::OP_RESID || op == pamg::OP_JACOBI || op >= 4) && !b) return fail(PAMG_E_ARG, "bench_rowop: b needed");
    if ((op == pamg::OP_JACOBI || op >= 4) && !A->d_diag)
        return fail(PAMG_E_SETUP, "bench_rowop: jacobi needs a square matrix");
    if (op == pamg::OP_CHEB) {  // one Chebyshev step k >= 1: c1 = c2 = omega, x_{k-1} a zeroed vector of the call's
        if (A->interior.pnc || A->interior.rpat) return fail(PAMG_E_ARG, "bench_rowop: op 6 needs a square operator");
        if (x == y || b == y) return fail(PAMG_E_ARG, "bench_rowop: y must differ from x and b");
        CHECK(check_vec_for(A, x, "bench_rowop"));
        if (b->n_own != A->nrows || y->n_own != A->nrows) return fail(PAMG_E_ARG, "bench_rowop: size mismatch");
        CHECK(set_device(ctx));
        double* xo = nullptr;
        CHECK(dalloc(&xo, A->nrows + kVecPad));
        int rc = dzero(ctx, xo, sizeof(double) * (size_t)(A->nrows + kVecPad));
        hipStream_t s = ctx->s_comp;
        if (rc == PAMG_OK)
            rc = time_reps(s, reps, avg_ms, [&]() {
                pamg::launch_rows(*A, A->interior, op, x->d, b->d, xo, y->d, omega, s, omega);
                pamg::launch_rows(*A, A->boundary, op, x->d, b->d, xo, y->d, omega, s, omega);
                return PAMG_OK;
            });
        dfree(xo);
        return rc;
    }
    if (op >= 4 && !(A->interior.sym && (A->sym.tb_ok || A->sym.tb_part)))
        return fail(PAMG_E_STATE, "bench_rowop: op %d needs the temporally blocked layout (pamg_mat_layout bit 5)", op);
    // (launch_sym has no prolongate-add: the layout is never built for a P; a launch would leave y as it was)
    if (op == pamg::OP_PROLONG && (A->interior.sym || A->boundary.sym))
        return fail(PAMG_E_STATE, "bench_rowop: the symmetric layouts have no prolongate-add kernel");
    if (x == y) return fail(PAMG_E_ARG, "bench_rowop: x and y must differ");
    CHECK(check_vec_for(A, x, "bench_rowop"));
    // a part's blocked passes (sweeps_part) feed each stage's output to the next stage's boundary
    // rows, which read its ghost slots: y and the scratch stages need the column length
    const bool part_tb = op >= 4 && A->sym.tb_part;
    if (part_tb) CHECK(check_vec_for(A, y, "bench_rowop (y: input of the next stage)"));
    CHECK(set_device(ctx));
    // ops 4 / 5: the temporally blocked passes k_sym_tb<2> (Jacobi -> residual) and <3>
    // (Jacobi -> Jacobi -> residual), the first output into y, the others into scratch
    double* scratch[2] = {nullptr, nullptr};
    int rc = PAMG_OK;
    if (op >= 4) {
        const int64_t len = part_tb ? (A->plan ? A->plan->n_own + A->plan->n_ghost : A->ncols) : A->nrows;
        for (double*& p : scratch) {
            if (rc == PAMG_OK) rc = dalloc(&p, std::max<int64_t>(len, A->nrows) + kVecPad);
            if (rc == PAMG_OK) rc = dzero(ctx, p, sizeof(double) * (size_t)(std::max<int64_t>(len, A->nrows) + kVecPad));
        }
    }
    pamg::TbArgs ta;
    ta.nstages = op - 2;
    ta.last_resid = true;
    ta.in0 = x->d;
    // op 5 on one part mirrors the pipeline's chain (launch_chain3): its stage-0 output is stored
    // only with chain_store_x (a part's passes feed it to the edge planes: always stored there)
    ta.out[0] = op == 5 && !part_tb && !pamg::options().chain_store_x ? nullptr : y->d;
    ta.out[1] = scratch[0];
    ta.out[2] = scratch[1];
    ta.b = b ? b->d : nullptr;
    ta.omega = omega;
    hipStream_t s = ctx->s_comp;
    const double* bd = b ? b->d : nullptr;
    if (rc == PAMG_OK)
        rc = time_reps(s, reps, avg_ms, [&]() {
            if (op >= 4 && A->sym.tb_part)  // one part of several: its blocked pass + edge planes + boundary rows
                return sweeps_part(ctx, A, op - 2, x->d, ta.out, ta.b, omega, false);
            if (op >= 4) {
                pamg::launch_sym_tb(*A, ta, s);
            } else {
                pamg::launch_set(*A, A->interior, op, x->d, bd, x->d, y->d, omega, s);
                pamg::launch_set(*A, A->boundary, op, x->d, bd, x->d, y->d, omega, s);
            }
            return (int)PAMG_OK;
        });
    for (double* p : scratch) dfree(p);
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ several right-hand sides (SPEC §S13)
// A multi-column operation is k independent single-column operations. One function per kind of step
// decides how the columns run: where the operator is in the block-row layout, launch_bsr_multi streams the
// matrix once for up to four columns; everywhere else the columns go one after the other through the
// single-column launchers above, with the column pointers offset. One part only.

namespace {

using pamg::mc::kMaxCols;

// The columns of one operand of a multi-column step (any subset of a multi-vector's columns)
struct Cols {
    double* p[kMaxCols] = {};
};

Cols cols_of(double* base, int64_t stride, int k) {
    Cols c;
    for (int j = 0; j < k; ++j) c.p[j] = base + (int64_t)j * stride;
    return c;
}
Cols cols_of(const pamg_vec* v) { return cols_of(v->d, v->stride, v->ncols); }

// columns at[0 .. m - 1] of c
Cols subset(const Cols& c, const int* at, int m) {
    Cols out;
    for (int j = 0; j < m; ++j) out.p[j] = c.p[at[j]];
    return out;
}

// y_c = op(A, x_c[, b_c]) for k columns: apply's bits per column
int apply_multi(pamg_ctx* ctx, const pamg_mat* A, int op, int k, const Cols& x, const Cols* b, const Cols& y,
                double omega, double c1 = 0.0, const Cols* xold = nullptr) {
    if (k > 1 && pamg::bsr_any(*A)) {
        // (a block-row operator has no ghost column: nothing to exchange)
        if ((op == pamg::OP_CHEB || op == pamg::OP_JACOBI) && !A->d_diag && A->nrows > 0)
            return fail(PAMG_E_ARG, "jacobi / chebyshev: a square operator with a nonzero diagonal is needed");
        pamg::launch_bsr_multi(*A, op, 0, k, x.p, b ? b->p : nullptr, xold ? xold->p : nullptr, y.p, omega, c1,
                               ctx->s_comp);
        HIPC(hipGetLastError());
        return PAMG_OK;
    }
    for (int c = 0; c < k; ++c)
        CHECK(apply(ctx, A, op, x.p[c], b ? b->p[c] : nullptr, y.p[c], omega, c1, xold ? xold->p[c] : nullptr));
    return PAMG_OK;
}

// smooth_step on k columns (in and xold null where the step names none)
int smooth_step_multi(pamg_ctx* ctx, const pamg_mat* A, bool blk, plan::Op op, int k, const Cols* in, const Cols& b,
                      const Cols* xold, const Cols& out, double c1, double c2) {
    hipStream_t s = ctx->s_comp;
    if (!(k > 1 && A->interior.bsr)) {
        for (int c = 0; c < k; ++c)
            CHECK(smooth_step(ctx, A, blk, op, in ? in->p[c] : nullptr, b.p[c], xold ? xold->p[c] : nullptr, out.p[c], c1,
                              c2));
        return PAMG_OK;
    }
    if (blk) {  // block_step's three forms
        const int mode = op == plan::CHEB ? pamg::BM_CHEB : op == plan::SMOOTH ? pamg::BM_JACOBI : pamg::BM_ZERO;
        if (mode == pamg::BM_ZERO) {
            for (int c = 0; c < k; ++c) pamg::launch_block_update(*A, mode, b.p[c], nullptr, nullptr, out.p[c], 0.0, c2, s);
        } else if (pamg::bsr_fused(*A)) {
            pamg::launch_bsr_multi(*A, pamg::OP_RESID, mode == pamg::BM_JACOBI ? 1 : 2, k, in->p, b.p,
                                   xold ? xold->p : nullptr, out.p, c2, c1, s);
        } else {
            CHECK(apply_multi(ctx, A, pamg::OP_RESID, k, *in, &b, out, 0.0));
            for (int c = 0; c < k; ++c)
                pamg::launch_block_update(*A, mode, out.p[c], in->p[c], xold ? xold->p[c] : nullptr, out.p[c], c1, c2, s);
        }
        HIPC(hipGetLastError());
        return PAMG_OK;
    }
    if (op == plan::CHEB) return apply_multi(ctx, A, pamg::OP_CHEB, k, *in, &b, out, c2, c1, xold);
    if (op == plan::SMOOTH) return apply_multi(ctx, A, pamg::OP_JACOBI, k, *in, &b, out, c2);
    for (int c = 0; c < k; ++c) pamg::launch_jacobi_zero(A->nrows, b.p[c], A->d_diag, c2, out.p[c], s);
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// ghost capacity of level l's vectors (pamg_hier_create's rule)
int64_t level_ghosts(const pamg_hier* H, int l) {
    int64_t g = 0;
    if (H->A[l]->plan) g = std::max(g, H->A[l]->plan->n_ghost);
    if (l < H->L - 1 && H->R[l]->plan) g = std::max(g, H->R[l]->plan->n_ghost);
    if (l > 0 && H->P[l - 1]->plan) g = std::max(g, H->P[l - 1]->plan->n_ghost);
    return g;
}

int alloc_cols(pamg_ctx* ctx, double** p, int k, int64_t stride) {
    const int64_t n = (int64_t)k * stride + kVecPad;
    CHECK(dalloc(p, n));
    return dzero(ctx, *p, sizeof(double) * (size_t)n);
}

// The hierarchy's work vectors in k columns: allocated on the first multi-column call, grown (and the
// cycle's graph dropped) when a later call brings more columns.
int ensure_multi(pamg_hier* H, int k) {
    if (k <= H->mc_cols) return PAMG_OK;
    pamg_ctx* ctx = H->ctx;
    HIPC(hipStreamSynchronize(ctx->s_comp));
    drop_multi_graph(H);
    free_multi(H);
    const int L = H->L;
    H->mc_stride.assign(L, 0);
    for (std::vector<double*>* set : {&H->mx, &H->mb, &H->mt, &H->mr}) set->assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        H->mc_stride[l] = pamg::mc::col_stride(H->nown[l], level_ghosts(H, l));
        if (l > 0) {
            CHECK(alloc_cols(ctx, &H->mx[l], k, H->mc_stride[l]));
            CHECK(alloc_cols(ctx, &H->mb[l], k, H->mc_stride[l]));
        }
        if (l < L - 1) {
            CHECK(alloc_cols(ctx, &H->mt[l], k, H->mc_stride[l]));
            CHECK(alloc_cols(ctx, &H->mr[l], k, H->mc_stride[l]));
        }
    }
    H->mc_cols = k;
    return PAMG_OK;
}

// the multi-column cycle's plan: pamg_vcycle's without the temporally blocked level-0 pass (same bits)
plan::CycleSpec cycle_spec_multi(const pamg_hier* H, bool zero0) {
    plan::CycleSpec sp = cycle_spec(H, zero0);
    sp.l0_fused = false;
    return sp;
}

// vcycle_enqueue on k columns: the same plan::plan_cycle step list, the roles resolved per column.
// Not profiled (pamg_hier_profile ignores multi-column calls).
int vcycle_enqueue_multi(pamg_hier* H, int k, const Cols& x, const Cols& b, bool zero0) {
    pamg_ctx* ctx = H->ctx;
    hipStream_t s = ctx->s_comp;
    const int L = H->L;
    if (L == 1) {
        for (int c = 0; c < k; ++c) CHECK(coarse_solve(H, b.p[c], x.p[c], s));
        HIPC(hipGetLastError());
        return PAMG_OK;
    }
    const plan::CyclePlan cp = plan::plan_cycle(cycle_spec_multi(H, zero0));
    if (cp.needs_u0 && !H->mu0) return fail(PAMG_E_STATE, "vcycle_multi: the cycle lacks its spare level-0 vector");
    auto vec = [&](int l, plan::Role r) -> Cols {
        if (l == 0 && r == plan::X) return x;
        if (l == 0 && r == plan::B) return b;
        double* const v[5] = {H->mx[l], H->mb[l], H->mt[l], H->mr[l], H->mu0};
        return cols_of(v[r], H->mc_stride[l], k);
    };
    for (const plan::Step& st : cp.steps) {
        const int l = st.level;
        const Cols bl = vec(l, plan::B);
        Cols in, xo;
        if (st.in != plan::NONE) in = vec(st.op == plan::PROLONG ? l + 1 : l, st.in);
        if (st.xold != plan::NONE) xo = vec(l, st.xold);
        const Cols out = vec(l, st.out);
        switch (st.op) {
            case plan::RESID:
                CHECK(apply_multi(ctx, H->A[l], pamg::OP_RESID, k, in, &bl, out, 0.0));
                break;
            case plan::JACOBI_RESID:
                return fail(PAMG_E_STATE, "vcycle_multi: the plan names a temporally blocked pass");
            case plan::RESTRICT:
                CHECK(apply_multi(ctx, H->R[l], pamg::OP_SPMV, k, in, nullptr, vec(l + 1, plan::B), 0.0));
                break;
            case plan::COARSE:
                for (int c = 0; c < k; ++c) CHECK(coarse_solve(H, in.p[c], out.p[c], s));
                break;
            case plan::PROLONG:
                CHECK(apply_multi(ctx, H->P[l], pamg::OP_PROLONG, k, in, nullptr, out, 0.0));
                break;
            default: {
                double c1, c2;
                smooth_coeffs(H, l, st.k, &c1, &c2);
                CHECK(smooth_step_multi(ctx, H->A[l], block_level(H, l), st.op, k, st.in == plan::NONE ? nullptr : &in, bl,
                                        st.xold == plan::NONE ? nullptr : &xo, out, c1, c2));
            }
        }
    }
    HIPC(hipGetLastError());
    return PAMG_OK;
}

// ncycles multi-column cycles on the columns x / b (stride sx / sb apart): graph replay when enabled, one
// exec keyed on the two bases, their strides, the column count and the zero-guess flag.
int vcycle_multi_raw(pamg_hier* H, int k, double* x, int64_t sx, double* b, int64_t sb, int ncycles, bool zero0) {
    pamg_ctx* ctx = H->ctx;
    CHECK(ensure_multi(H, k));
    if (H->L > 1 && !H->mu0 && plan::plan_cycle(cycle_spec_multi(H, zero0)).needs_u0)
        CHECK(alloc_cols(ctx, &H->mu0, H->mc_cols, H->mc_stride[0]));
    const Cols xc = cols_of(x, sx, k), bc = cols_of(b, sb, k);
    // (the strides ride in the key as the distance of column 1: the bases alone do not tell two layouts apart)
    const double* kx = x + sx;
    const double* kb = b + sb;
    if (H->use_graph && (!H->gm_exec || H->gm_x != x || H->gm_b != b || H->gm_k != k || H->gm_zero0 != zero0 ||
                         H->gm_x1 != kx || H->gm_b1 != kb)) {
        drop_multi_graph(H);
        if (capture_graph(ctx->s_comp, [&] { return vcycle_enqueue_multi(H, k, xc, bc, zero0); }, &H->gm_exec)) {
            H->gm_x = x;
            H->gm_b = b;
            H->gm_x1 = kx;
            H->gm_b1 = kb;
            H->gm_k = k;
            H->gm_zero0 = zero0;
        } else {
            H->gm_exec = nullptr;
            capture_failed(H, "multi-column V-cycle");
        }
    }
    if (H->use_graph && H->gm_exec) {
        for (int j = 0; j < ncycles; ++j) HIPC(hipGraphLaunch(H->gm_exec, ctx->s_comp));
    } else {
        for (int j = 0; j < ncycles; ++j) CHECK(vcycle_enqueue_multi(H, k, xc, bc, zero0 && j == 0));
    }
    return PAMG_OK;
}

// The k-wide reduction workspace beside ctx->d_red
int ensure_redk(pamg_ctx* ctx) {
    if (ctx->d_redk) return PAMG_OK;
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_redk), kMaxCols * sizeof(double)));
    return dalloc(&ctx->d_redk, (int64_t)kMaxCols * 1024 + kMaxCols);
}

// m deterministic sums of one step: enqueue(j, np, partials, result, stream) puts sum j's partial and
// final kernels on the compute stream (launch_dot's grid and trees, its own partials), then the host
// waits once for all of them.
template <class F>
int reduce_multi(pamg_ctx* ctx, int64_t n, int m, double* out, F enqueue) {
    hipStream_t s = ctx->s_comp;
    const int np = pamg::dot_partials(n);
    if (np > 1024 || m > kMaxCols) return fail(PAMG_E_STATE, "reduction workspace too small");
    if (m <= 0) return PAMG_OK;
    CHECK(ensure_redk(ctx));
    double* res = ctx->d_redk + (int64_t)kMaxCols * 1024;
    for (int j = 0; j < m; ++j) enqueue(j, np, ctx->d_redk + (int64_t)j * 1024, res + j, s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(ctx->h_redk, res, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (int j = 0; j < m; ++j) out[j] = ctx->h_redk[j];
    return PAMG_OK;
}

int dots_multi(pamg_ctx* ctx, int64_t n, int m, const Cols& x, const Cols& y, double* out) {
    return reduce_multi(ctx, n, m, out, [&](int j, int np, double* parts, double* res, hipStream_t s) {
        pamg::launch_dot(n, x.p[j], y.p[j], parts, np, res, s);
    });
}

bool cols_ok(const pamg_vec* v) { return v->ncols >= 1 && v->ncols <= kMaxCols; }

// do the allocations of two multi-vectors (or column views) share memory?
bool overlap(const pamg_vec* a, const pamg_vec* b) {
    const double* a1 = a->d + (int64_t)a->ncols * a->stride;
    const double* b1 = b->d + (int64_t)b->ncols * b->stride;
    return a == b || (a->d < b1 && b->d < a1);
}

// the checks every multi-column entry point on a matrix shares
int check_multi_op(pamg_ctx* ctx, const pamg_mat* A, const pamg_vec* X, const pamg_vec* B, const pamg_vec* Y,
                   const char* who) {
    if (ctx->nranks > 1) return fail(PAMG_E_STATE, "%s: one part only (SPEC §S13)", who);
    if (!cols_ok(X) || !cols_ok(Y) || (B && !cols_ok(B))) return fail(PAMG_E_ARG, "%s: need 1..8 columns", who);
    if (X->ncols != Y->ncols || (B && B->ncols != X->ncols))
        return fail(PAMG_E_ARG, "%s: the column counts disagree (%d, %d, %d)", who, X->ncols, B ? B->ncols : X->ncols,
                    Y->ncols);
    CHECK(check_vec_for(A, X, who));
    if (Y->n_own != A->nrows || (B && B->n_own != A->nrows)) return fail(PAMG_E_ARG, "%s: size mismatch", who);
    if (overlap(X, Y) || (B && (overlap(X, B) || overlap(B, Y))))
        return fail(PAMG_E_ARG, "%s: the multi-vectors must not alias", who);
    return PAMG_OK;
}

// the checks the two hierarchy entry points share
int check_multi_hier(pamg_ctx* ctx, const pamg_hier* H, const pamg_vec* X, const pamg_vec* B, const char* who) {
    if (ctx->nranks > 1) return fail(PAMG_E_STATE, "%s: one part only (SPEC §S13)", who);
    if (H->d_perm)
        return fail(PAMG_E_STATE, "%s: not on a hierarchy with a level-0 permutation (pamg_hier_set_perm)", who);
    if (!cols_ok(X) || !cols_ok(B)) return fail(PAMG_E_ARG, "%s: need 1..8 columns", who);
    if (X->ncols != B->ncols)
        return fail(PAMG_E_ARG, "%s: X has %d columns, B %d", who, X->ncols, B->ncols);
    CHECK(check_vec_for(H->A[0], X, who));
    if (B->n_own != H->A[0]->nrows) return fail(PAMG_E_ARG, "%s: B size mismatch", who);
    if (overlap(X, B)) return fail(PAMG_E_ARG, "%s: X and B must not alias", who);
    return PAMG_OK;
}

}  // namespace

extern "C" {

int pamg_mvec_create(pamg_ctx* ctx, int64_t n_own, int64_t n_ghost, int ncols, pamg_vec** out) {
    if (!ctx || !out || n_own < 0 || n_ghost < 0) return fail(PAMG_E_ARG, "mvec_create: bad args");
    if (ncols < 1 || ncols > kMaxCols) return fail(PAMG_E_ARG, "mvec_create: %d columns outside 1..%d", ncols, kMaxCols);
    CHECK(set_device(ctx));
    std::unique_ptr<pamg_vec, int (*)(pamg_vec*)> v(new pamg_vec, pamg_vec_destroy);
    v->ctx = ctx;
    ctx_ref(ctx);
    v->n_own = n_own;
    v->n_ghost = n_ghost;
    v->ncols = ncols;
    v->stride = pamg::mc::col_stride(n_own, n_ghost);
    CHECK(alloc_cols(ctx, &v->d, ncols, v->stride));
    *out = v.release();
    return PAMG_OK;
}

int pamg_mvec_destroy(pamg_vec* mv) { return pamg_vec_destroy(mv); }

int pamg_mvec_size(const pamg_vec* mv, int64_t* n_own, int64_t* n_ghost, int* ncols, int64_t* stride) {
    if (!mv) return fail(PAMG_E_ARG, "mvec_size: NULL");
    if (n_own) *n_own = mv->n_own;
    if (n_ghost) *n_ghost = mv->n_ghost;
    if (ncols) *ncols = mv->ncols;
    if (stride) *stride = mv->stride;
    return PAMG_OK;
}

int pamg_mvec_upload(pamg_ctx* ctx, pamg_vec* mv, const double* own) {
    if (!ctx || !mv || (!own && mv->n_own)) return fail(PAMG_E_ARG, "mvec_upload: bad args");
    CHECK(set_device(ctx));
    if (mv->n_own)
        HIPC(hipMemcpy2DAsync(mv->d, sizeof(double) * mv->stride, own, sizeof(double) * mv->n_own,
                              sizeof(double) * mv->n_own, mv->ncols, hipMemcpyHostToDevice, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_mvec_download(pamg_ctx* ctx, const pamg_vec* mv, double* own) {
    if (!ctx || !mv || (!own && mv->n_own)) return fail(PAMG_E_ARG, "mvec_download: bad args");
    CHECK(set_device(ctx));
    if (mv->n_own)
        HIPC(hipMemcpy2DAsync(own, sizeof(double) * mv->n_own, mv->d, sizeof(double) * mv->stride,
                              sizeof(double) * mv->n_own, mv->ncols, hipMemcpyDeviceToHost, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_mvec_column(pamg_vec* mv, int c, pamg_vec** view) {
    if (!mv || !view) return fail(PAMG_E_ARG, "mvec_column: bad args");
    if (c < 0 || c >= mv->ncols) return fail(PAMG_E_ARG, "mvec_column: column %d of %d", c, mv->ncols);
    pamg_vec* v = new pamg_vec;
    v->ctx = mv->ctx;
    ctx_ref(mv->ctx);
    v->n_own = mv->n_own;
    v->n_ghost = mv->n_ghost;
    v->d = mv->d + (int64_t)c * mv->stride;
    v->stride = mv->stride;
    v->owns = false;
    *view = v;
    return PAMG_OK;
}

int pamg_spmm(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* X, pamg_vec* Y) {
    if (!ctx || !A || !X || !Y) return fail(PAMG_E_ARG, "spmm: NULL");
    CHECK(check_multi_op(ctx, A, X, nullptr, Y, "spmm"));
    CHECK(set_device(ctx));
    CHECK(apply_multi(ctx, A, pamg::OP_SPMV, X->ncols, cols_of(X), nullptr, cols_of(Y), 0.0));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_residual_multi(pamg_ctx* ctx, const pamg_mat* A, pamg_vec* X, const pamg_vec* B, pamg_vec* R, double* nrm2) {
    if (!ctx || !A || !X || !B || !R) return fail(PAMG_E_ARG, "residual_multi: NULL");
    CHECK(check_multi_op(ctx, A, X, B, R, "residual_multi"));
    CHECK(set_device(ctx));
    const int k = X->ncols;
    const Cols b = cols_of(B), r = cols_of(R);
    CHECK(apply_multi(ctx, A, pamg::OP_RESID, k, cols_of(X), &b, r, 0.0));
    if (nrm2) {
        double rr[kMaxCols];
        CHECK(dots_multi(ctx, R->n_own, k, r, r, rr));
        for (int c = 0; c < k; ++c) nrm2[c] = std::sqrt(rr[c]);
    }
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_vcycle_multi(pamg_ctx* ctx, pamg_hier* H, pamg_vec* X, const pamg_vec* B, int ncycles, double* res_hist) {
    if (!ctx || !H || !X || !B || ncycles < 0 || H->ctx != ctx) return fail(PAMG_E_ARG, "vcycle_multi: bad args");
    CHECK(check_multi_hier(ctx, H, X, B, "vcycle_multi"));
    CHECK(set_device(ctx));
    const int k = X->ncols;
    if (!res_hist) {
        CHECK(vcycle_multi_raw(H, k, X->d, X->stride, B->d, B->stride, ncycles, false));
        HIPC(hipStreamSynchronize(ctx->s_comp));
        return PAMG_OK;
    }
    CHECK(ensure_multi(H, k));
    // r = b - A x into the level-0 residual columns (a one-level hierarchy has none: a temporary)
    double* tmp = nullptr;
    const int64_t n = H->nown[0], rs = H->mc_stride[0];
    if (H->L == 1) CHECK(alloc_cols(ctx, &tmp, k, rs));
    const Cols x = cols_of(X), b = cols_of(B), r = cols_of(H->L > 1 ? H->mr[0] : tmp, rs, k);
    int rc = PAMG_OK;
    for (int j = 0; j < ncycles && rc == PAMG_OK; ++j) {
        rc = vcycle_multi_raw(H, k, X->d, X->stride, B->d, B->stride, 1, false);
        if (rc == PAMG_OK) rc = apply_multi(ctx, H->A[0], pamg::OP_RESID, k, x, &b, r, 0.0);
        double rr[kMaxCols];
        if (rc == PAMG_OK) rc = dots_multi(ctx, n, k, r, r, rr);
        for (int c = 0; c < k && rc == PAMG_OK; ++c) res_hist[(size_t)j * k + c] = std::sqrt(rr[c]);
    }
    if (tmp) {
        (void)hipStreamSynchronize(ctx->s_comp);
        dfree(tmp);
    }
    CHECK(rc);
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}

int pamg_pcg_multi(pamg_ctx* ctx, pamg_hier* H, pamg_vec* X, const pamg_vec* B, double rtol, int maxit, int* iters,
                   double* res_hist) {
    if (!ctx || !H || !X || !B || maxit < 0 || !(rtol >= 0.0) || H->ctx != ctx)
        return fail(PAMG_E_ARG, "pcg_multi: bad args");
    CHECK(check_multi_hier(ctx, H, X, B, "pcg_multi"));
    CHECK(set_device(ctx));
    const pamg_mat* A = H->outer ? H->outer : H->A[0];
    const int k = X->ncols;
    const int64_t n = A->nrows;
    CHECK(ensure_multi(H, k));
    const int64_t ws = H->mc_stride[0];
    if (!H->mpcg_r)
        for (double** p : {&H->mpcg_r, &H->mpcg_z, &H->mpcg_p, &H->mpcg_q}) CHECK(alloc_cols(ctx, p, H->mc_cols, ws));
    hipStream_t s = ctx->s_comp;
    const Cols x = cols_of(X), b = cols_of(B);
    const Cols r = cols_of(H->mpcg_r, ws, k), z = cols_of(H->mpcg_z, ws, k), p = cols_of(H->mpcg_p, ws, k),
               q = cols_of(H->mpcg_q, ws, k);
    const size_t hl = (size_t)maxit + 1;
    double rr[kMaxCols], nr0[kMaxCols], rz[kMaxCols], tmp[kMaxCols];
    int it[kMaxCols] = {};
    CHECK(apply_multi(ctx, A, pamg::OP_RESID, k, x, &b, r, 0.0));
    CHECK(dots_multi(ctx, n, k, r, r, rr));
    // the running columns, in column order; a column leaves when it has stopped (SPEC §S13)
    int act[kMaxCols], m = 0;
    for (int c = 0; c < k; ++c) {
        nr0[c] = std::sqrt(rr[c]);
        if (res_hist) res_hist[c * hl] = nr0[c];
        if (nr0[c] > 0.0 && maxit > 0) act[m++] = c;
    }
    if (m > 0) {
        // z = M^-1 r on all k columns (a stopped column rides along, its z is ignored): one graph
        CHECK(vcycle_multi_raw(H, k, H->mpcg_z, ws, H->mpcg_r, ws, 1, true));
        for (int j = 0; j < m; ++j)
            HIPC(hipMemcpyAsync(p.p[act[j]], z.p[act[j]], sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        CHECK(dots_multi(ctx, n, m, subset(r, act, m), subset(z, act, m), tmp));
        for (int j = 0; j < m; ++j) rz[act[j]] = tmp[j];
        for (int step = 1; step <= maxit && m > 0; ++step) {
            const Cols pa = subset(p, act, m), qa = subset(q, act, m), xa = subset(x, act, m), ra = subset(r, act, m);
            CHECK(apply_multi(ctx, A, pamg::OP_SPMV, m, pa, nullptr, qa, 0.0));
            CHECK(dots_multi(ctx, n, m, pa, qa, tmp));
            double alpha[kMaxCols];
            for (int j = 0; j < m; ++j) alpha[j] = rz[act[j]] / tmp[j];
            // x += alpha p; r -= alpha q; rr = r.r per column (launch_cg_update's shape), one wait
            CHECK(reduce_multi(ctx, n, m, tmp, [&](int j, int np, double* parts, double* res, hipStream_t st) {
                pamg::launch_cg_update(n, alpha[j], pa.p[j], qa.p[j], xa.p[j], ra.p[j], parts, np, res, st);
            }));
            int keep = 0;
            for (int j = 0; j < m; ++j) {
                const int c = act[j];
                const double nr = std::sqrt(tmp[j]);
                it[c] = step;
                if (res_hist) res_hist[c * hl + step] = nr;
                if (!(nr <= rtol * nr0[c])) act[keep++] = c;
            }
            m = keep;
            if (m == 0 || step == maxit) break;
            CHECK(vcycle_multi_raw(H, k, H->mpcg_z, ws, H->mpcg_r, ws, 1, true));
            CHECK(dots_multi(ctx, n, m, subset(r, act, m), subset(z, act, m), tmp));
            for (int j = 0; j < m; ++j) {
                const int c = act[j];
                const double beta = tmp[j] / rz[c];
                rz[c] = tmp[j];
                pamg::launch_axpby(n, 1.0, z.p[c], beta, p.p[c], s);
            }
        }
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    if (iters)
        for (int c = 0; c < k; ++c) iters[c] = it[c];
    return PAMG_OK;
}

int pamg_bench_rowop_multi(pamg_ctx* ctx, const pamg_mat* A, int op, pamg_vec* X, const pamg_vec* B, pamg_vec* Y,
                           double omega, int reps, double* avg_ms) {
    const bool known = (op >= 0 && op <= 3) || (op >= 6 && op <= 8);
    if (!ctx || !A || !X || !Y || reps < 1 || !avg_ms || !known) return fail(PAMG_E_ARG, "bench_rowop_multi: bad args");
    const bool needs_b = op == pamg::OP_RESID || op == pamg::OP_JACOBI || op >= 6;
    if (needs_b && !B) return fail(PAMG_E_ARG, "bench_rowop_multi: B needed");
    if (!needs_b) B = nullptr;
    CHECK(check_multi_op(ctx, A, X, B, Y, "bench_rowop_multi"));
    if ((op == pamg::OP_JACOBI || op == pamg::OP_CHEB) && !A->d_diag)
        return fail(PAMG_E_SETUP, "bench_rowop_multi: jacobi needs a square matrix");
    if (op == pamg::OP_CHEB && (A->interior.pnc || A->interior.rpat))
        return fail(PAMG_E_ARG, "bench_rowop_multi: op 6 needs a square operator");
    if (op >= 7) CHECK(check_block_op(A, "bench_rowop_multi"));
    if (op == pamg::OP_PROLONG && (A->interior.sym || A->boundary.sym))
        return fail(PAMG_E_STATE, "bench_rowop_multi: the symmetric layouts have no prolongate-add kernel");
    CHECK(set_device(ctx));
    const int k = X->ncols;
    double* zero = nullptr;  // x_{k-1} of ops 6 and 8
    const int64_t zs = pamg::mc::col_stride(A->nrows, 0);
    if (op == pamg::OP_CHEB || op == 8) CHECK(alloc_cols(ctx, &zero, k, zs));
    const Cols x = cols_of(X), y = cols_of(Y), b = B ? cols_of(B) : Cols{}, xo = zero ? cols_of(zero, zs, k) : Cols{};
    const int rc = time_reps(ctx->s_comp, reps, avg_ms, [&]() {
        if (op == 7) return smooth_step_multi(ctx, A, true, plan::SMOOTH, k, &x, b, nullptr, y, 0.0, omega);
        if (op == 8) return smooth_step_multi(ctx, A, true, plan::CHEB, k, &x, b, &xo, y, omega, omega);
        return apply_multi(ctx, A, op, k, x, B ? &b : nullptr, y, omega, omega, op == pamg::OP_CHEB ? &xo : nullptr);
    });
    dfree(zero);
    return rc;
}

}  // extern "C"
