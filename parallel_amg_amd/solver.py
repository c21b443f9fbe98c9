"""Device AMG solver: uploads one part of a ``HostHierarchy`` and runs V-cycles (SPEC §S6).

``AMGSolver`` is the preconditioner object an AMG-on-PartitionedArrays driver would pass
around (``ldiv!``-style ``vcycle``); the cycle itself is one C-ABI call (``pamg_vcycle``),
replayed as a hipGraph on one part.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import call, ptr
from .hcsr import block_diag, gen_xstar
from .hierarchy import SEED, HostHierarchy
from .partitioned import (Context, MultiVector, PSparseMatrix, PVector, _release, estimate_lmax,
                          estimate_lmax_block)

OPS = ("jacobi_pre", "residual", "restrict", "prolong", "jacobi_post", "coarse")


REORDER = {"off": 0, "auto": 1, "on": 2, "agg": 3}


def plan_tag(level: int, op: str) -> int:
    """Tag of a hierarchy's column plan (pamg_plan_set_tag): 1 + 3 level + (A 0, P 1, R 2)."""
    return 1 + 3 * int(level) + "APR".index(op)


class _LevelOps:
    """Read-only sequence view of an AMGSolver's level operators: index 0 resolves through
    ``fine_operator()`` (the caller's numbering), every other index is ``A_dev[l]``."""

    def __init__(self, solver):
        self._s = solver

    def __len__(self):
        return len(self._s.A_dev)

    def __getitem__(self, l):
        if isinstance(l, slice):
            return [self[i] for i in range(*l.indices(len(self)))]
        l = range(len(self))[l]
        return self._s.fine_operator() if l == 0 else self._s.A_dev[l]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class AMGSolver:
    def __init__(self, ctx: Context, H: HostHierarchy, part: int = 0, graph: bool | None = None,
                 reorder: str = "auto", block_layout=None, values: str = "f64"):
        """``block_layout``: None, a block size (level 0) or a ``{level: block size}`` dict — those
        levels' operators are uploaded through pamg_mat_upload_blocked and, where they qualify (every
        node's rows store the same whole blocks, one part without ghost columns), run in the
        block-row layout: every result keeps its bits, and a point-block sweep (``set_block_size`` with
        the same size, then a block smoother) is one pass over the matrix instead of two. Such a
        level must stay unpermuted (ValueError otherwise: build with ``reorder="off"``, and renumber
        the nodes before setup). Which to take ("Block-row layout"; one MI355X, 80^3 nodes of
        three unknowns, PCG to 1e-8 with block Chebyshev V(2,2), ``lmax="estimate"``): take it for
        vector-valued operators whose values do not repeat (finite elements, variable coefficients),
        most of all where the numbering is not a grid's — 10.8 ms against 14.9 on a randomly
        renumbered variable-coefficient operator, 7.70 against 7.87 in grid order, the iteration
        counts equal. Do not take it for a constant-coefficient grid operator like elastic3d: its
        four distinct values fit the dictionary tiles, which stream a seventh of the bytes (18.3 ms
        against 37.8 with the block-row layout).

        On a nodal hierarchy (``SAParams(block_size=bs)``, SPEC §S14) every level keeps node structure:
        ``block_layout="all"`` uploads every A_l through pamg_mat_upload_blocked and every P_l and R_l
        through pamg_mat_upload_block_rows with the hierarchy's block size (ValueError on a hierarchy
        built with ``block_size=1``); ``{"A": {...}, "P": {...}, "R": {...}}`` names the levels of each
        (``{level: block size}``, as above). The multi-column cycle then streams every operator once per
        chunk of columns. Which to take: DESIGN.md, "Nodal hierarchy".

        ``reorder`` (one part only): a locality permutation of every level but the coarsest
        inside the device layout (pamg_locality_order / pamg_mat_upload_perm): "auto" takes
        reverse Cuthill-McKee on the levels whose numbering is scattered (FE meshes, random
        renumberings and the levels aggregated from them), "on" on every level, "off" never.
        A_l, P_l and R_l are uploaded through the fine and coarse permutations with each row
        in its storage order, and the V-cycle gathers / scatters the caller's level-0 vectors
        (pamg_hier_set_perm), so every result keeps the unpermuted hierarchy's bits.

        ``values="f32"`` (SPEC §S15; the default "f64" is the path above, untouched): the V-cycle runs on
        ``hierarchy.round_values(H)`` — every A_l, P_l and R_l rounded to binary32, uploaded with
        ``value_bits=32``, so the levels in the block-row layout (``block_layout``) stream 4-byte values — while
        ``pcg`` and ``pcg_multi`` solve with the exact A_0: it is uploaded once more in fp64 (in the block-row
        layout where level 0 has it) and set as the outer operator (``set_fine_operator``). ``fine_operator()``
        and ``A[0]`` return the exact operator, ``A_dev[0]`` the rounded one; ``set_block_size`` and
        ``estimate_lmax`` read the rounded matrices, the weights and bounds stay the fp64 setup's. A stationary
        ``vcycle`` iterates on the rounded A_0. Cost in memory: level 0 is held 1.5 times (the fp64 copy beside
        the 4-byte one). Level 0 must stay unpermuted (ValueError: ``reorder="off"``); a permuted coarser level
        goes through the permuted fp64 upload with its values already rounded: it is the rounded operator, stored
        in fp64, and its ``value_bits`` reads 64 (the mark is the f32 upload's; the permuted upload has none). ValueError where a value overflows binary32. Which to take
        ("Single-precision values"; one MI355X, 80^3 nodes of three unknowns with variable
        coefficients, PCG to 1e-8 with block Jacobi V(1,1), ``lmax="estimate"``): take it together with
        ``block_layout`` when PCG is the solver — 6.29 ms against 7.22 in grid order and 9.96 against 11.16 with the
        nodes renumbered at random, 7 and 8 iterations either way, the same final residual; a level-0 pass takes
        0.61 and 0.76 of its fp64 time. Without ``block_layout`` nothing stores 4-byte values and nothing gets
        faster. On the nodal hierarchy it gains the same 13 % (20.5 ms against 23.5) and does not mend that
        hierarchy's loss against the scalar one."""
        if values not in ("f64", "f32"):
            raise ValueError(f"values: {values!r} ('f64' or 'f32')")
        self.values = values
        H_exact = H
        if values == "f32":
            from .hierarchy import round_values
            H = round_values(H)
        vbits = 32 if values == "f32" else 64
        self.ctx, self.part, self.L = ctx, part, H.nlevels
        # the level operators as the hierarchy holds them (device numbering where permuted);
        # ``A`` (below) gives level 0 in the caller's numbering
        self.A_dev, self.P, self.R, self.omega = [], [], [], []
        self._A0_caller = None
        self._H = H
        # levels >= rep are whole on every part (agglomerated tail / coarsest level): the
        # prolongation into rep - 1 reads that whole vector, so its columns stay global
        rep = H.rep_level if H.nparts > 1 else H.nlevels - 1
        mode = REORDER[reorder]
        if H.nparts > 1 and mode == 2:
            raise ValueError("reorder='on' needs a one-part hierarchy (renumber a partitioned "
                             "matrix before setup: partition='rcm')")
        # per level: device row i = host row perm[l][i] (None: identity); the coarsest level
        # keeps its numbering (its dense inverse sums in column order)
        self.perm = [None] * H.nlevels
        self.span = [None] * H.nlevels
        if H.nparts == 1 and mode == REORDER["agg"]:
            # levels 1 .. L-2 in the order of their coarse aggregates: the nodes
            # of one level-(l+1) aggregate become a contiguous run — R_l's rows read runs of the
            # level-l vector instead of ~25 scattered lines — each aggregate's nodes in their own
            # order, the aggregates in coarse-row order; level 0 keeps its grid layout
            for l in range(1, H.nlevels - 1):
                agg = H.levels[l][part].agg
                if agg is None or len(agg) != H.levels[l][part].A.nrows:
                    continue
                agg = np.asarray(agg, np.int64)
                key = np.where(agg < 0, np.int64(1) << 40, agg)
                self.perm[l] = np.argsort(key, kind="stable").astype(np.int64)
        elif H.nparts == 1 and mode:
            from .hcsr import locality_order
            for l in range(H.nlevels - 1):
                order, before, after = locality_order(H.levels[l][part].A, mode)
                self.perm[l] = order
                self.span[l] = (round(before, 1), round(after, 1))
        if values == "f32" and self.perm[0] is not None:
            raise ValueError("values='f32': level 0 is uploaded with a locality permutation, which the outer "
                             "operator does not take (build the solver with reorder='off')")
        transfers = {"P": {}, "R": {}}
        if isinstance(block_layout, str):
            if block_layout != "all":
                raise ValueError(f"block_layout: {block_layout!r} (a block size, a dict or 'all')")
            hbs = int(getattr(H, "block_size", 1))
            if hbs == 1:
                raise ValueError("block_layout='all' needs a nodal hierarchy (SAParams(block_size=bs), SPEC §S14): "
                                 "this one was built with block_size=1")
            block_layout = {l: hbs for l in range(H.nlevels)}
            transfers = {w: {l: hbs for l in range(H.nlevels - 1)} for w in ("P", "R")}
        elif isinstance(block_layout, dict) and any(isinstance(k, str) for k in block_layout):
            if set(block_layout) - {"A", "P", "R"}:
                raise ValueError(f"block_layout: keys {sorted(map(str, block_layout))} (levels, or 'A', 'P' and 'R')")
            transfers = {w: dict(block_layout.get(w) or {}) for w in ("P", "R")}
            block_layout = dict(block_layout.get("A") or {})
        if block_layout is None:
            block_layout = {}
        elif not isinstance(block_layout, dict):
            block_layout = {0: block_layout}
        self.block_layout = {range(H.nlevels)[int(l)]: int(bs) for l, bs in block_layout.items() if int(bs) != 1}
        # the transfers in the block-row layout (pamg_mat_upload_block_rows): level -> block size
        self.block_layout_P, self.block_layout_R = (
            {range(H.nlevels - 1)[int(l)]: int(bs) for l, bs in transfers[w].items() if int(bs) != 1}
            for w in ("P", "R"))
        for which, lay in (("A", self.block_layout), ("P", self.block_layout_P), ("R", self.block_layout_R)):
            for l, bs in lay.items():
                if bs < 1 or bs > 4:
                    raise ValueError(f"block_layout: block size {bs} of level {l} outside 1..4")
                if self.perm[l] is not None or (which != "A" and self.perm[l + 1] is not None):
                    raise ValueError(f"block_layout: level {l} is uploaded with a locality permutation, which the "
                                     "block-row layout does not take (build the solver with reorder='off' and "
                                     "renumber the nodes before setup)")
        for l in range(H.nlevels):
            lp = H.levels[l][part]
            pl = self.perm[l]
            pn = self.perm[l + 1] if l + 1 < H.nlevels else None
            # plan tags (pamg_plan_set_tag): level and operator, the same on every part
            # (a permuted level of a values="f32" hierarchy: its rounded values through the fp64 upload)
            self.A_dev.append(PSparseMatrix(ctx, lp.A, lp.planA, row_perm=pl, col_perm=pl, tag=plan_tag(l, "A"),
                                            block_size=self.block_layout.get(l, 1),
                                            value_bits=64 if pl is not None else vbits))
            self.omega.append(lp.omega)
            if l < H.nlevels - 1:
                self.P.append(PSparseMatrix(ctx, lp.P, None if l + 1 >= rep else lp.planP,
                                            row_perm=pl, col_perm=pn, tag=plan_tag(l, "P"),
                                            block_rows=self.block_layout_P.get(l, 1),
                                            value_bits=64 if pl is not None or pn is not None else vbits))
                self.R.append(PSparseMatrix(ctx, lp.R, lp.planR, row_perm=pn, col_perm=pl, tag=plan_tag(l, "R"),
                                            block_rows=self.block_layout_R.get(l, 1),
                                            value_bits=64 if pl is not None or pn is not None else vbits))
        self.level_rows = [int(H.levels[l][part].A.nrows) for l in range(H.nlevels)]
        self.n_coarse = H.n_coarse
        L = self.L
        arrA = (C.c_void_p * L)(*[a.handle for a in self.A_dev])
        arrP = (C.c_void_p * L)(*([p.handle for p in self.P] + [None]))
        arrR = (C.c_void_p * L)(*([r.handle for r in self.R] + [None]))
        om = np.asarray(self.omega, np.float64)
        roffs = np.asarray(H.rep_offsets, np.int64) if H.nparts > 1 else None
        self.rep_level = rep
        self._ainv = np.ascontiguousarray(H.ainv, np.float64)
        h = C.c_void_p()
        call("pamg_hier_create", ctx.handle, L, arrA, arrP, arrR, ptr(om), H.n_coarse,
             ptr(self._ainv), int(rep), ptr(roffs) if roffs is not None else None, C.byref(h))
        self._h = h
        self.smoother = "jacobi"
        self.last_pcg_stats = None
        # point blocks (set_block_size): level -> block size, and level -> rho_b = ||D_b^-1 A_l||_inf
        self.block_size, self.rho_b = {}, {}
        if self.perm[0] is not None:
            p0 = np.ascontiguousarray(self.perm[0], np.int64)
            call("pamg_hier_set_perm", h, len(p0), ptr(p0))
        if graph is not None:
            self.set_graph(graph)
        self._outer = None
        if values == "f32":
            lp = H_exact.levels[0][part]
            self.set_fine_operator(PSparseMatrix(ctx, lp.A, lp.planA, dplan=self.A_dev[0].plan,
                                                 block_size=self.block_layout.get(0, 1)))

    def set_fine_operator(self, A: PSparseMatrix | None):
        """The operator ``pcg`` and ``pcg_multi`` form b - A x and A p with (pamg_hier_set_outer, SPEC §S15),
        and ``fine_operator()`` / ``A[0]`` return: the exact fp64 A_0 around a hierarchy of rounded operators.
        ``None`` restores the hierarchy's own level 0. A has level 0's shape and shares its column plan
        (``PSparseMatrix(..., dplan=solver.A_dev[0].plan)``); PamgError otherwise, and on a hierarchy whose
        level 0 is permuted. The V-cycle, and a stationary ``vcycle``'s residual history, stay level 0's own."""
        call("pamg_hier_set_outer", self._h, A.handle if A is not None else None)
        self._outer = A

    @property
    def A(self) -> "_LevelOps":
        """The level operators, level 0 in the CALLER's numbering (b = A[0] x, residuals of the
        caller's vectors): the hierarchy's own A_0 when level 0 is not permuted, else an
        unpermuted upload made on first use of index 0 (``fine_operator``; ADVICE r4: ``A[l]``
        for l >= 1 never triggers it). Levels >= 1 are internal to the cycle and listed as the
        hierarchy holds them (``A_dev``)."""
        return _LevelOps(self)

    @property
    def reordered(self) -> list:
        """Levels whose device layout carries a locality permutation."""
        return [l for l, p in enumerate(self.perm) if p is not None]

    def fine_operator(self) -> PSparseMatrix:
        """The level-0 operator in the caller's numbering (for b = A x and residuals of the
        caller's vectors): the hierarchy's own A_0 when level 0 is not permuted, else an
        unpermuted upload (made once, kept)."""
        if self._outer is not None:
            return self._outer
        if self.perm[0] is None:
            return self.A_dev[0]
        if self._A0_caller is None:
            lp = self._H.levels[0][self.part]
            self._A0_caller = PSparseMatrix(self.ctx, lp.A, lp.planA)
        return self._A0_caller

    @property
    def handle(self):
        return self._h

    def set_graph(self, enable: bool):
        call("pamg_hier_set_graph", self._h, int(bool(enable)))

    def set_sweeps(self, nu1: int, nu2: int):
        """V(nu1, nu2) weighted-Jacobi sweeps (SPEC §S6; default V(1, 1))."""
        call("pamg_hier_set_sweeps", self._h, int(nu1), int(nu2))

    def set_block_size(self, bs: int, levels=(0,), backend=None):
        """Attach point-block data of ``bs`` unknowns per node (2..4; SPEC §S12) to the operators of
        ``levels`` — row ``bs m + d`` is unknown d of node m — for the "block_jacobi" and
        "block_chebyshev" smoothers; ``bs = 1`` removes it. The default is level 0 alone: scalar-strength
        aggregation mixes a node's unknowns, so coarser levels have no node structure. On a nodal
        hierarchy (SPEC §S14) every level has: ``levels="all"`` names every level but the coarsest. Raises
        ValueError for a level whose device layout is permuted (``reorder``) or whose part offsets are
        not multiples of ``bs``. ``self.rho_b[l]`` keeps ||D_b^-1 A_l||_inf, the maximum over the parts
        this process holds, or over all of them through ``backend.allreduce_max``. Call
        ``set_smoother`` afterwards."""
        bs = int(bs)
        if isinstance(levels, str):
            if levels != "all":
                raise ValueError(f"set_block_size: levels {levels!r} (level numbers or 'all')")
            levels = range(self.L - 1)
        for l in levels:
            l = range(self.L - 1)[l]
            A = self.A_dev[l]
            if bs == 1:
                A.set_block_diag(1)
                self.block_size.pop(l, None)
                self.rho_b.pop(l, None)
                continue
            if self.perm[l] is not None:
                raise ValueError(f"set_block_size: level {l} is uploaded with a locality permutation "
                                 "(build the solver with reorder='off')")
            offs = np.asarray(self._H.levels[l][self.part].offsets, np.int64)
            if bs < 2 or bs > 4:
                raise ValueError(f"set_block_size: block size {bs} outside 1..4")
            if np.any(offs % bs):
                raise ValueError(f"set_block_size: the part offsets {offs.tolist()} of level {l} are not "
                                 f"multiples of {bs}")
            rho, mine = {}, None
            for p, lp in self._H.levels[l].items():
                row0 = 0 if lp.whole else int(lp.offsets[p])
                blocks, inv, rho[p] = block_diag(lp.A, row0, bs)
                if p == self.part:
                    mine = (blocks, inv)
            A.set_block_diag(bs, *mine)
            self.block_size[l] = bs
            self.rho_b[l] = float(backend.allreduce_max(rho)) if backend is not None else max(rho.values())

    def estimate_lmax(self, steps: int = 10, boost: float = 1.1, seed: int = SEED, block: bool | None = None):
        """Device estimate of lambda_max(D^-1 A_l) for every level but the coarsest (SPEC §S10):
        ``steps`` power-iteration steps from the §S2 generator vector of seed ``seed + l`` (global
        row numbering), then lmax_l = min(rho_l, boost * lambda_steps). Returns the L-1 values and
        keeps the raw lambda histories in ``self.lmax_hist``. Collective on several parts: every
        part calls it, and every part gets the same values. ``block`` (default: whether a block
        smoother is active): the levels with block data (``set_block_size``) estimate
        lambda_max(D_b^-1 A_l) instead, capped by ``rho_b[l]`` (SPEC §S12)."""
        if block is None:
            block = self.smoother in ("block_jacobi", "block_chebyshev")
        out, self.lmax_hist = [], []
        for l in range(self.L - 1):
            A, lp = self.A_dev[l], self._H.levels[l][self.part]
            whole = l >= self.rep_level
            i0 = 0 if whole else int(lp.offsets[self.part])
            v, y = A.new_input_vector(), A.new_output_vector()
            if self.perm[l] is None:
                v.fill_xstar(i0, seed + l)
            else:  # device row i is host row perm[i]: the generator values in the device numbering
                v.set(gen_xstar(i0, A.nrows, seed + l)[self.perm[l]])
            blk = block and l in self.block_size
            lam = (estimate_lmax_block if blk else estimate_lmax)(A, v, y, steps, all_parts=not whole)
            self.lmax_hist.append(lam)
            out.append(min(self.rho_b[l] if blk else lp.rho, boost * float(lam[-1])))
        return out

    def set_smoother(self, kind: str = "jacobi", ratio: float = 4.0, lmax="gershgorin"):
        """The V-cycle's smoother: "jacobi" (default) or "chebyshev" — one polynomial of degree nu1
        before and nu2 after the coarse correction (``set_sweeps`` gives the degrees), level l over
        [lmax_l / ratio, lmax_l] (SPEC §S9). ``lmax``: "gershgorin" (the setup's bound rho_l,
        ``LevelPart.rho``), "estimate" (``estimate_lmax()`` with its defaults, SPEC §S10) or a
        sequence of L-1 floats. For Jacobi a non-default ``lmax`` sets the weights
        omega_l = 4 / (3 lmax_l) (pamg_hier_set_omega); "gershgorin" restores the setup's.

        "block_jacobi" / "block_chebyshev" (SPEC §S12; after ``set_block_size``): the same cycle with
        D_b^-1, the inverse node blocks, for D^-1 on the levels with block data, and the scalar
        smoother of the same kind on the others. There "gershgorin" means ``rho_b[l]`` (so block
        Jacobi's default weight is 4 / (3 rho_b)), "estimate" the block estimate capped by it, and
        a sequence is taken as given. Each block sweep is the layout's residual pass plus one vector
        pass (+17 % on a level-0 sweep of elastic3d 80^3), or a single fused pass on a level in the
        block-row layout (``AMGSolver(..., block_layout=bs)``). Which to take ("Point-block
        smoothers"; one MI355X, elastic3d 80^3, PCG to 1e-8, ``lmax="estimate"``): block Jacobi V(1,1)
        18.7 ms / 36 iterations against 23.8 / 47 for Jacobi, block Chebyshev V(2,2) 18.1 / 26 against
        19.9 / 30 — the best solve measured; at V(3,3) the block form loses (20.1 / 23 against
        19.6 / 24). Use the block forms with "estimate": rho_b = 2.0 is 1.4 times the spectrum's top,
        and with it block Jacobi V(1,1) needs 49 iterations."""
        kinds = {"jacobi": 0, "chebyshev": 1, "block_jacobi": 2, "block_chebyshev": 3}
        if kind not in kinds:
            raise ValueError(f"unknown smoother {kind!r} (jacobi | chebyshev | block_jacobi | block_chebyshev)")
        nl = self.L - 1
        block = kinds[kind] >= 2
        if block and not self.block_size:
            from ._lib import PamgError
            raise PamgError(-6, "set_smoother", "a block smoother needs block data: call set_block_size first")
        jac = kind in ("jacobi", "block_jacobi")
        if isinstance(lmax, str):
            if lmax not in ("gershgorin", "estimate"):
                raise ValueError(f"unknown lmax {lmax!r} (gershgorin | estimate | a sequence of {nl} floats)")
            bound = self.estimate_lmax(block=block) if lmax == "estimate" else None
        else:
            bound = [float(v) for v in lmax]
            if len(bound) != nl:
                raise ValueError(f"lmax needs {nl} entries, got {len(bound)}")
        # the Jacobi weights: 4 / (3 lmax_l) (the expression of SPEC §S4.1) for Jacobi with a bound
        # of its own, else the setup's — so "jacobi" without lmax is the setup's cycle again
        if bound is not None and jac:
            omega = [4.0 / (3.0 * v) for v in bound]
        else:
            omega = [float(w) for w in self.omega[:nl]]
            if block:  # the default weight of a block level comes from its own bound
                for l in self.block_size:
                    omega[l] = 4.0 / (3.0 * self.rho_b[l])
        if bound is None:
            bound = [self.rho_b[l] if block and l in self.block_size else self._H.levels[l][self.part].rho
                     for l in range(nl)]
        lm, om = np.asarray(bound, np.float64), np.asarray(omega, np.float64)
        call("pamg_hier_set_smoother", self._h, kinds[kind], None if jac else ptr(lm), float(ratio))
        call("pamg_hier_set_omega", self._h, ptr(om))
        self.smoother = kind
        self.lmax = list(bound)

    def graph_state(self) -> dict:
        e, c, f = C.c_int(), C.c_int(), C.c_int()
        call("pamg_hier_graph_state", self._h, C.byref(e), C.byref(c), C.byref(f))
        return {"enabled": bool(e.value), "captured": bool(c.value), "failed": bool(f.value)}

    def new_vector(self) -> PVector:
        """A level-0 vector with room for the fine-level ghosts."""
        return self.A_dev[0].new_input_vector()

    def vcycle(self, x: PVector, b: PVector, ncycles: int = 1, res_hist: bool = False):
        if res_hist:
            hist = np.zeros(ncycles)
            call("pamg_vcycle", self.ctx.handle, self._h, x.handle, b.handle, ncycles, ptr(hist))
            return hist
        call("pamg_vcycle", self.ctx.handle, self._h, x.handle, b.handle, ncycles, None)
        return None

    def pcg(self, x: PVector, b: PVector, rtol: float = 1e-8, maxit: int = 100, lookahead: int | None = None):
        """CG preconditioned by one V-cycle (SPEC §S8); returns (iterations, ||r_k|| history).

        ``lookahead=None`` (default) is ``pamg_pcg``: the scalars on the host, three waits per
        iteration. An integer takes ``pamg_pcg_resident`` (SPEC §S11, one part only): the scalars stay
        in device memory and the iteration is replayed as two graphs, with the same bits in x, the
        count and the history. ``0`` waits once per iteration and runs nothing past convergence;
        ``L >= 1`` waits only for iteration j - L's outcome and runs up to L iterations (a V-cycle
        each) past convergence. ``self.last_pcg_stats`` then holds (iterations enqueued, of those
        after convergence); it is None after a ``lookahead=None`` call.

        Which to take ("Device-resident PCG"; one MI355X, rtol 1e-8): where an iteration
        is shorter than about a millisecond (poisson3d 128^3, elastic3d 80^3) ``lookahead=0`` is
        3-4 % faster than ``None``; at 512^3 (8 ms per iteration) the two are level. ``L >= 1`` was
        never faster than ``0`` — the stream is already fed — and pays its L late iterations: 7-23 %
        on solves of 9-19 iterations, 1-3 % on 39-66. Use ``0`` for short iterations, ``None`` or
        ``0`` for long ones, and ``L >= 1`` only where the host thread answers waits slowly."""
        hist = np.zeros(maxit + 1)
        it = C.c_int()
        if lookahead is None:
            self.last_pcg_stats = None
            call("pamg_pcg", self.ctx.handle, self._h, x.handle, b.handle, float(rtol), int(maxit),
                 C.byref(it), ptr(hist))
        else:
            stats = (C.c_int * 2)()
            call("pamg_pcg_resident", self.ctx.handle, self._h, x.handle, b.handle, float(rtol), int(maxit),
                 int(lookahead), C.byref(it), ptr(hist), stats)
            self.last_pcg_stats = (int(stats[0]), int(stats[1]))
        return it.value, hist[: it.value + 1]

    def new_multivector(self, ncols: int) -> MultiVector:
        """``ncols`` level-0 vectors in one ``MultiVector`` (SPEC §S13), zeroed."""
        return MultiVector(self.ctx, self.A_dev[0].n_own_cols, ncols, self.A_dev[0].n_ghost)

    def vcycle_multi(self, X: MultiVector, B: MultiVector, ncycles: int = 1, res_hist: bool = False):
        """``vcycle`` on every column of X (SPEC §S13; ``pamg_vcycle_multi``): each column gets the bits
        of ``vcycle`` on that column alone. With ``res_hist`` returns the ``(ncycles, k)`` residual norms.
        One part, no level-0 permutation (``reorder="off"``). Where level 0 is in the block-row layout
        (``block_layout``), its passes stream the matrix once for up to four columns."""
        if res_hist:
            hist = np.zeros((ncycles, X.ncols))
            call("pamg_vcycle_multi", self.ctx.handle, self._h, X.handle, B.handle, ncycles, ptr(hist))
            return hist
        call("pamg_vcycle_multi", self.ctx.handle, self._h, X.handle, B.handle, ncycles, None)
        return None

    def pcg_multi(self, X: MultiVector, B: MultiVector, rtol: float = 1e-8, maxit: int = 100):
        """``pcg`` on every column of X (SPEC §S13; ``pamg_pcg_multi``): each column runs its own CG —
        own scalars, own stopping test — and stops on its own; returns (the k iteration counts, the k
        residual histories), each column's the bits of ``pcg(lookahead=None)`` on that column alone.
        Which to take ("Several right-hand sides"; one MI355X, elastic3d_var 80^3 with level 0 in
        the block-row layout, against k separate ``pcg`` calls): in grid order 2 / 4 / 8 columns take 0.74 /
        0.60 / 0.60 of the time; with the nodes renumbered at random, where the x gathers bound the passes,
        0.86 / 0.91 / 0.91 — there two columns per call serve best. Without a block-row level 0 every step
        loops over the columns and only the host waits are shared."""
        k = X.ncols
        hist = np.zeros((k, maxit + 1))
        it = np.zeros(k, np.int32)
        call("pamg_pcg_multi", self.ctx.handle, self._h, X.handle, B.handle, float(rtol), int(maxit), ptr(it), ptr(hist))
        return it.astype(np.int64), [hist[c, : it[c] + 1].copy() for c in range(k)]

    def vcycle_async(self, x: PVector, b: PVector, ncycles: int = 1):
        call("pamg_vcycle_async", self.ctx.handle, self._h, x.handle, b.handle, ncycles)

    def bench_chain(self, x: PVector, b: PVector, reps: int = 10):
        """ms per launch of the cross-cycle pipeline's level-0 chain kernel (None when the
        hierarchy does not run the pipeline); x is overwritten."""
        from ._lib import PamgError
        ms = C.c_double()
        try:
            call("pamg_hier_bench_chain", self._h, x.handle, b.handle, int(reps), C.byref(ms))
        except PamgError:
            return None
        return ms.value

    def profile(self, x: PVector, b: PVector, ncycles: int) -> np.ndarray:
        """Eager V-cycles with HIP events around every op; returns ms per (level, op) summed
        over the cycles (shape L x 6, columns = OPS)."""
        call("pamg_hier_profile", self._h, 1)
        try:
            call("pamg_vcycle_async", self.ctx.handle, self._h, x.handle, b.handle, ncycles)
            out = np.zeros(self.L * 6)
            call("pamg_hier_profile_read", self._h, ptr(out))
        finally:
            call("pamg_hier_profile", self._h, 0)
        return out.reshape(self.L, 6)

    # ---- algorithmic byte model (SURVEY.md §8d / BASELINE.md) --------------------------
    @staticmethod
    def rowsum_bytes(M, extra_vec_rw: int) -> int:
        """Algorithmic bytes of one row operation of the device matrix M: the
        matrix stream in its uploaded layout (pamg_mat_stream_bytes: 8 B values + 4 B, or 3 B
        in 24-bit column tiles, columns per nonzero + row pointers + tile descriptors) + 8 B per
        x entry read once + 8 B per output row + 8 B per extra own vector read or written."""
        return M.stream_bytes + 8 * (M.n_own_cols + M.n_ghost) + 8 * M.nrows + 8 * M.nrows * extra_vec_rw

    @staticmethod
    def csr_bytes(M, extra_vec_rw: int) -> int:
        """SURVEY §8(d)'s algorithmic bytes of one row operation, independent of the device
        layout: plain CSR with 32-bit indices (12 B per nonzero + 4 B per row pointer) + 8 B
        per x entry read once + 8 B per output row + 8 B per extra own vector read or written
        (b; the diagonal is read inline). The layouts libpamg uploads (24-bit columns, 8-bit
        row lengths, column dictionaries) stream fewer bytes than this (rowsum_bytes)."""
        return (12 * M.nnz + 4 * (M.nrows + 1) + 8 * (M.n_own_cols + M.n_ghost) + 8 * M.nrows
                + 8 * M.nrows * extra_vec_rw)

    def op_bytes(self, model: str = "format") -> np.ndarray:
        """Bytes per (level, op) of one V-cycle on this part (L x 6): model "format" = what
        the uploaded layout streams (rowsum_bytes), "csr" = SURVEY §8(d)'s CSR model."""
        rb = self.rowsum_bytes if model == "format" else self.csr_bytes
        out = np.zeros((self.L, 6))
        for l in range(self.L):
            n = self.level_rows[l]
            if l == self.L - 1:
                nc = self.n_coarse
                out[l, 5] = 8 * nc * n + 8 * nc + 8 * n
                continue
            A, P, R = self.A_dev[l], self.P[l], self.R[l]
            # jacobi: x (read once), b, x' ; zero-guess form on l >= 1 reads b, diag, writes x'
            out[l, 0] = rb(A, 1) if l == 0 else 24 * n
            out[l, 1] = rb(A, 1)
            out[l, 2] = rb(R, 0)
            out[l, 3] = rb(P, 1)
            out[l, 4] = rb(A, 1)
        return out

    def __del__(self):
        _release(self, "pamg_hier_destroy")
