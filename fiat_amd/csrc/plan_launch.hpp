// The planner of the simplex tabulation: which of the five kernel families takes a request (generic, cooperative,
// shape-specialised image / stream / pair, lane-local, stacked with the request-per-workgroup kernel), with which registry
// row and which launch geometry.  A section of api.hip, included there once, below the registries it reads:
//
//   validate -> Request -> generic item shape -> choose_coop -> choose_fixed -> choose_small -> choose_stacked
//            -> pick the winner -> fill_<winner>
//
// A choose_* does integer work on the Request and on the choices of the stages before it: it never sees pts / verts / out and
// writes nothing into the Launch.  A fill_* writes the argument struct and the Launch fields of its family from the choice, for
// the winner only.  A new window goes into the choose_* of the family that TAKES the shape -- into the predicate of the stacked
// kind for a stacked row -- and, where another family has to give the shape up, into the named yield predicate of that family
// (small_keeps / over_small / fixed_yields, stacked_pio_ok), with its measurement in the comment above it.
#pragma once

namespace {

// ---- the request: what every stage reads, built once after validation ---------------------------------------------------
struct Request {
    fx_ctx* ctx;
    const fx_element* e;
    unsigned policy;
    int num_cu, lds_per_cu;
    int order;
    long long nreq;
    int npts;
    bool has_cells;  // per-request cells (`verts`)
    int mapping;     // FX_MAP_*
    int ntab, rows;
    long long R;     // stacked rows = ntab * rows
    int RT;          // ... in row tiles
    bool even;       // the stacked tables leave in 16-byte pieces (odd_tables)
    // The caller wants the element's Piola map fused into the tabulation.  ONE predicate for the four stages: the cooperative,
    // shape-specialised and lane-local stages used to write it without `sd >= 2`, but their registries have no row below
    // sd 2 (registries_at_least_2d below), so the term never decided anything there; the stacked probe had it.  (sd 1 with a
    // Piola map: fx_tabulate_batch_mapped refuses it; fx_plan_kernel passes it on unchecked -- an interval element has vdim
    // 1 = sd, so the old lane-local form was true there and met no row.)
    bool want_piola;
    bool pio_even, pio_odd_twin;  // parity of the tables on the Piola twins' row tiles; the point windows of the two odd twins
    bool stacked_pio_ok;          // the stacked kernel applies the map itself: the cooperative and lane-local kernels leave it the shape
    int debug;                    // FIAT_AMD_DEBUG of the measurement build
    bool has(unsigned policy_bits) const { return (policy & policy_bits) != 0; }
};

constexpr bool registries_at_least_2d() {
    for (const CoopShape& c : kCoopShapes)
        if (c.sd < 2) return false;
    for (const FixedShape& f : kFixedShapes)
        if (f.sd < 2) return false;
    for (const SmallShape& s : kSmallShapes)
        if (s.sd < 2) return false;
    return true;
}
static_assert(registries_at_least_2d(), "Request::want_piola holds `sd >= 2` for every stage: no registry row may be 1-D");

Request make_request(fx_ctx* ctx, const fx_element* e, int order, int64_t nreq, int npts, bool has_cells, int mapping) {
    Request rq{};
    rq.ctx = ctx;
    rq.e = e;
    rq.policy = ctx->policy;
    rq.num_cu = ctx->num_cu;
    rq.lds_per_cu = ctx->lds_per_cu;
    rq.order = order;
    rq.nreq = nreq;
    rq.npts = npts;
    rq.has_cells = has_cells;
    rq.mapping = mapping;
    rq.ntab = fx::binom(e->sd + order, e->sd);
    rq.rows = e->ndof * e->vdim;
    rq.R = (long long)rq.ntab * rq.rows;
    rq.RT = (int)((rq.R + 15) / 16);
    rq.even = !odd_tables(rq.R, npts);
    // the element's Piola map asked for with the tabulation, and can the stacked kernel apply it to its accumulators (PIO
    // instances: whole requests of <= 48 points, even table sizes)?  Then the cooperative and the lane-local kernel leave
    // their fused variants of these shapes to it (coverage map with the map: N2 tetrahedra at 11 points, gradients,
    // 14 % of the HBM peak on the cooperative kernel against 37 %; N3 triangles 29 % lane-local against 50 %)
    rq.want_piola = (mapping == FX_MAP_COVARIANT_PIOLA || mapping == FX_MAP_CONTRAVARIANT_PIOLA) && has_cells && e->vdim == e->sd && e->sd >= 2;
    const int TRp = fxk::stacked_tile_rows(e->sd, 1);
    rq.pio_even = !odd_tables(rq.rows, npts, TRp);
    // (odd table sizes: 8-byte twins of the two instances RT2 / N3 tetrahedra meet at their 11- / 23-point rules)
    rq.pio_odd_twin = e->sd == 3 && ((e->n == 2 && npts > 8 && npts <= 12) || (e->n == 3 && npts > 16 && npts <= 24));
    // ... and is there a row of the order's kind with a Piola twin that holds THIS request, by the predicates of the selection
    // loop below -- without the probe the cooperative and the lane-local kernel gave up their fused variants for shapes no
    // stacked instance then took (N2 / RT2 tetrahedra at <= 8 points: generic kernel + a separate push-forward pass)
    bool pio_instance = false;
    for (const StackedShape& k : kStackedShapes)
        pio_instance = pio_instance || (k.sd == e->sd && k.n == e->n && k.rtc == (order == 0 ? -6 : order == 1 ? -2 : -3) && k.pio &&
                                        holds_request(k, npts) && fills_tiles(k, npts));
    rq.stacked_pio_ok = rq.want_piola && !rq.has(FX_POLICY_NO_STACKED | FX_POLICY_NO_STACKED_MIX) && !e->raw_expansion &&
                        npts <= 48 && (rq.pio_even || rq.pio_odd_twin) && (long long)rq.ntab * rq.rows >= 15 &&
                        pio_instance && order <= 2;
    if (const char* dbg = ab_env("FIAT_AMD_DEBUG")) rq.debug = atoi(dbg);  // ablation switches (measurement only)
    return rq;
}

// ---- what a stage hands on: the registry row (id < 0: none) and the geometry it computed on the way --------------------
struct GenericShape {
    int P = 1, pc = 0, nchunk = 1;
    long long nitems = 0;
    int phi_doubles = 0, stage_doubles = 0, lds_bytes = 0;
};
struct CoopChoice {
    int id = -1;
    bool fuses = false;  // the row applies the Piola map in its output rounds
    int nt_need = 0, TR = 0, img_doubles = 0, lds_bytes = 0;
    double A0inv[9] = {};
};
struct FixedChoice {
    int id = -1;
    bool fuses = false;
    int fkind = 0, lds_doubles = 0, lds_bytes = 0, grid = 0;
};
struct SmallChoice {
    int id = -1;
    bool fuses = false;
    int P = 1;  // requests per wave
};
// the request-per-workgroup instance (rtc -7): only takes_workgroup fills it
struct WgFacts {
    int g = 1;         // requests per slab of <= 128 columns
    int ct = 0;        // column tiles of the instance
    bool mix = false;  // the order-1 chain rule of per-request cells on its accumulators (MIX instance)
    bool odd = false;  // 8-byte flush
};
struct StackedChoice {
    int id = -1;
    bool pio = false;      // the Piola twin
    bool mix_odd = false;  // the 8-byte twin of a chain-rule row
    bool kodd = false;     // Launch::kodd
    bool dofmajor = false;
    WgFacts wg;
    const double* afrag = nullptr;  // the element's stacked fragments the row reads (plain, dof-major, dof-major for the Piola twins)
    double A0inv[9] = {};
    int lds_bytes = 0, grid = 0;
    bool fixed_yields = false;  // the shape-specialised choice gives the request up to this one
};

// ---- the generic kernel's work-item shape under a per-wave LDS budget ----------------------------------------------------
int choose_generic_shape(const Request& rq, GenericShape& g) {
    const fx_element* e = rq.e;
    const int ntab = rq.ntab, npts = rq.npts;
    const long long budget = 32 * 1024;  // bytes per wave: >= 5 resident waves per CU
    // (hard limit: one wave's tile may take what a CU has -- the kernel runs one wave per workgroup; reached by expansion
    // degrees beyond 12 on tetrahedra, one column tile of 16 x nexp doubles: degree 16, 969 members, 124 KB)
    const long long hard = std::max<long long>(64 * 1024, (long long)rq.lds_per_cu - 4096);
    auto phi_bytes = [&](long long cols) { return ((cols + 15) / 16) * (long long)e->KS * 64 * 8; };
    const long long reqbytes = (long long)ntab * rq.rows * npts * 8;
    int P = 1, pc = npts, nchunk = 1;
    long long stage = 0;
    if (npts <= 64 && phi_bytes((long long)ntab * npts) + reqbytes <= budget) {
        // whole requests, output staged through LDS; pack as many as fit in a wave
        int pmax = 64 / npts;
        P = 1;
        for (int p = 2; p <= pmax; ++p)
            if (phi_bytes((long long)p * ntab * npts) + p * reqbytes <= budget) P = p;
        stage = P * reqbytes;
    } else {
        // point-chunked, direct stores
        pc = std::min(npts, 64);
        while (pc > 1 && phi_bytes((long long)ntab * pc) > budget) --pc;
        if (phi_bytes((long long)ntab * pc) > hard)
            return fail(FX_ENOTIMPL, "expansion degree too large for the LDS tile (nexp=%d, ntab=%d)", e->nexp, ntab);
        nchunk = (npts + pc - 1) / pc;
    }
    g.P = P;
    g.pc = pc;
    g.nchunk = nchunk;
    g.nitems = nchunk > 1 ? rq.nreq * nchunk : (rq.nreq + P - 1) / P;
    g.phi_doubles = (int)(phi_bytes((long long)P * ntab * pc) / 8);
    g.stage_doubles = (int)((stage / 8 + 1) & ~1LL);
    if (stage == 0) g.stage_doubles = 0;
    g.lds_bytes = (g.phi_doubles + g.stage_doubles) * 8;
    return FX_OK;
}

// ---- cooperative kernel for large shapes? ---------------------------------------------------------------------------------
int choose_coop(const Request& rq, CoopChoice& out) {
    const fx_element* e = rq.e;
    const int ntab = rq.ntab, rows = rq.rows, npts = rq.npts;
    const int rem = rows % 16;
    const bool split = rem != 0 && rem <= 12;
    const int mt16 = split ? rows / 16 : (rows + 15) / 16, m4 = split ? (rem + 3) / 4 : 0;
    const int nt_need = (ntab * npts + 15) / 16;
    if (rq.has(FX_POLICY_NO_COOP) || npts > 64 || !e->d_coop_eint) return FX_OK;
    for (size_t i = 0; i < sizeof(kCoopShapes) / sizeof(kCoopShapes[0]); ++i) {
        const CoopShape& c = kCoopShapes[i];
        if (c.sd != e->sd || c.order != rq.order || c.mt16 != mt16 || c.m4 != m4 || nt_need > 4 * c.tpw) continue;
        const bool piola = c.can_piola && rq.want_piola;
        if (c.piola_only && !piola) continue;
        if (piola && rq.stacked_pio_ok) continue;
        const int table = rows * npts;
        // tables per output round: as many as LDS holds next to the A fragments and the chain
        // state while two workgroups still fit a CU (fewer rounds = fewer workgroup barriers per
        // request); when one workgroup fills the CU anyway, whatever is left of its LDS
        const long long other = ((long long)(mt16 + m4) * e->coop_KS * 64 + 4LL * 4 * ntab * 32) * 8;
        long long img_budget = rq.lds_per_cu / 2 - other - 1024;
        if (img_budget < 16 * 1024) img_budget = std::min<long long>(rq.lds_per_cu - other - 1024, 56 * 1024);
        int TR = std::max(1, (int)(img_budget / ((long long)table * 8)));
        TR = std::min(TR, ntab);
        if (piola) {  // the fused flush writes pairs: every round a whole number of them, <= 4 per thread
            if ((table & 1) && (TR & 1)) TR = TR > 1 ? TR - 1 : 0;
            while (TR > 0 && (long long)TR * table > 2 * 512 * fxk::PIOLA_SLOTS) TR -= (table & 1) ? 2 : 1;
            if (TR <= 0 || (((long long)ntab * table) & 1)) continue;
            if ((table & 1) && (ntab % TR) % 2) continue;  // the last round must be even too
        }
        long long img = std::max<long long>(2LL * (nt_need * 64 + 128), (long long)TR * table);
        img = (img + 1) & ~1LL;
        if (npts > 32) continue;  // LDS-resident chain state holds 32 points
        long long ldsb = ((long long)(mt16 + m4) * e->coop_KS * 64 + img + 4LL * 4 * ntab * 32) * 8;
        if (ldsb > rq.lds_per_cu) continue;
        if (piola && !invert_small(e->sd, e->A0, out.A0inv)) return fail(FX_EINVAL, "degenerate cell");
        out.id = (int)i;
        out.fuses = piola;
        out.nt_need = nt_need;
        out.TR = TR;
        out.img_doubles = (int)img;
        out.lds_bytes = (int)ldsb;
        break;
    }
    return FX_OK;
}

// ---- shape-specialised kernel available? ------------------------------------------------------------------------------------
// A/B: the stacked kernel's small-shape instances instead (policy stacked_small)
bool stacked_small_ab(const Request& rq) { return rq.has(FX_POLICY_STACKED_SMALL) && !rq.has_cells && rq.mapping == FX_MAP_AFFINE; }

FixedChoice choose_fixed(const Request& rq, const CoopChoice& coop) {
    const fx_element* e = rq.e;
    const int ntab = rq.ntab, rows = rq.rows, npts = rq.npts;
    FixedChoice out;
    if (rq.has(FX_POLICY_NO_FIXED) || stacked_small_ab(rq) || npts > 64) return out;
    const int nt_need = (ntab * npts + 15) / 16;
    for (size_t i = 0; i < sizeof(kFixedShapes) / sizeof(kFixedShapes[0]); ++i) {
        const FixedShape& f = kFixedShapes[i];
        // (half-image shapes keep the tables of each half in their own tiles: one spare tile is fine)
        const bool nt_ok = f.nt == nt_need || (!f.fullimg && f.nt == nt_need + 1);
        if (f.sd != e->sd || f.n != e->n || f.order != rq.order || f.rows != rows || !nt_ok) continue;
        {   // the image of a flush round leaves as 16-byte pieces: an even number of doubles per round (and so per request)
            const int th = f.fullimg ? ntab : (ntab + 1) / 2;
            if (((long long)th * rows * npts) % 2 || ((long long)(ntab - th) * rows * npts) % 2) continue;
        }
        const bool fuse_here = rq.want_piola && f.can_piola;
        if (coop.fuses && !fuse_here) continue;  // the cooperative kernel fuses the map, this one cannot
        if (!f.matches(e->prog)) continue;
        const char* kk = rq.has(FX_POLICY_KERNEL_IMAGE) ? "image" : rq.has(FX_POLICY_KERNEL_STREAM) ? "stream" : nullptr;
        // default: K-streamed kernel, two requests per wave when the points of two requests fit
        // one wave (A/B: FX_POLICY_KERNEL_IMAGE | _STREAM)
        // (pair kernel: the tables of each output half must fit half of the column tiles)
        const bool pair_ok = npts <= 32 * (3 - f.rpw) && (f.fullimg || ntab == 1 ||
                                                          (f.nt % 2 == 0 && (f.nt / 2) * 16 >= ((ntab + 1) / 2) * npts));
        int fkind = pair_ok ? 2 : 1;
        if (kk && !strcmp(kk, "image") && !f.pair_only) fkind = 0;
        if (kk && !strcmp(kk, "stream") && !f.pair_only) fkind = 1;
        if (f.pair_only && fkind != 2) continue;
        if (kk && !strcmp(kk, "pair") && pair_ok) fkind = 2;
        long long need = std::max<long long>((long long)f.nt * e->KS * 64, (long long)ntab * rows * npts);
        need = (need + 1) & ~1LL;
        if (fkind >= 1) {
            // per wave: half image (>= the K-step slab that aliases it) + 64-double dump row
            const int th = (fkind == 2 && f.fullimg) ? ntab : (ntab + 1) / 2;
            long long per_wave =
                std::max<long long>((long long)th * rows * npts, (long long)f.nt * 64 * (fkind == 2 ? f.rpw : 1)) + 64;
            per_wave = (per_wave + 1) & ~1LL;
            int rem = rows % 16;
            bool split = rem != 0 && rem <= 12;
            int nfrag = ((split ? rows / 16 : (rows + 15) / 16) + (split ? (rem + 3) / 4 : 0)) * e->KS;
            const int lds_bytes = (int)((nfrag * 64 + per_wave * FIXED_NW) * 8);
            // registers bound the occupancy: ask for every workgroup the CU can hold
            long long want = (long long)rq.num_cu * 4;
            const long long units = fkind == 2 ? (rq.nreq + f.rpw - 1) / f.rpw : rq.nreq;  // requests or pairs, one per wave
            long long nwg = (units + FIXED_NW - 1) / FIXED_NW;
            if (lds_bytes > rq.lds_per_cu) continue;
            if (fuse_here && fkind != 2) continue;
            out.lds_doubles = (int)per_wave;
            out.lds_bytes = lds_bytes;
            out.grid = (int)std::max<long long>(1, std::min<long long>(nwg, fkind >= 2 ? nwg : want));
        } else {
            if (fuse_here) continue;
            // 8 waves per CU (2 workgroups of 4 waves): pad the request to 1/2 of the CU's LDS
            long long per_wave = std::max<long long>(need * 8, (long long)(rq.lds_per_cu / 8));
            per_wave &= ~15LL;
            if (per_wave < need * 8) per_wave = need * 8;
            const int lds_bytes = (int)(per_wave * FIXED_NW);
            if (lds_bytes > rq.lds_per_cu) continue;
            int wg_per_cu = std::max(1, rq.lds_per_cu / lds_bytes);
            long long want = (long long)rq.num_cu * wg_per_cu;
            long long nwg = (rq.nreq + FIXED_NW - 1) / FIXED_NW;
            out.lds_doubles = (int)(per_wave / 8);
            out.lds_bytes = lds_bytes;
            out.grid = (int)std::max<long long>(1, std::min<long long>(nwg, want));
        }
        out.id = (int)i;
        out.fkind = fkind;
        out.fuses = fuse_here;
        break;
    }
    return out;
}

// ---- low-order lane-local kernel? -------------------------------------------------------------------------------------------
SmallChoice choose_small(const Request& rq, const CoopChoice& coop, const FixedChoice& fixed) {
    const fx_element* e = rq.e;
    const int order = rq.order, rows = rq.rows, npts = rq.npts;
    SmallChoice out;
    const long long reqbytes8 = (long long)rq.ntab * rows * npts * 8;
    if (rq.has(FX_POLICY_NO_SMALL) || order > 2 || npts > 64 || rows > 96 || reqbytes8 > 16 * 1024 || !e->d_cmat) return out;
    for (size_t i = 0; i < sizeof(kSmallShapes) / sizeof(kSmallShapes[0]); ++i) {
        if (kSmallShapes[i].sd != e->sd || kSmallShapes[i].n != e->n) continue;
        const bool values_only_shape = kSmallShapes[i].values_only;
        if (values_only_shape && (order != 0 || rq.mapping != FX_MAP_AFFINE || e->vdim != 1 || rq.has(FX_POLICY_WG_SMALL | FX_POLICY_NO_SMALL_VALUES))) continue;
        if (values_only_shape && e->sd == 3 && npts > 16) continue;   // (P3 tetrahedra: up to the 14-point rule)
        if (!kSmallShapes[i].matches(e->prog) || (int)e->prog.steps.size() > fxk::SMALL_MAXSTEPS) continue;
        int P = std::max(1, 64 / npts);
        // (17-24 rows -- vector-valued degree-2 triangles -- with Hessians: 6.9 KB a request left ONE request a wave, six of 64 lanes
        // at the 6-point rule, and the shape went to the generic kernel at 31 % of the HBM peak; up to 28 KB a wave there)
        const long long image_cap = ((rows > 16 && e->sd == 2) || rows > 24) ? 28 * 1024 : 12 * 1024;   // (N1 tetrahedra, 18 rows, with Hessians: 199 us at two requests a wave, 213 at four)
        while (P > 1 && P * reqbytes8 > image_cap) --P;  // per-wave image: several workgroups per CU
        // many rows (vector-valued elements): the MFMA contraction of the generic / stacked kernels wins over
        // rows x members FMAs per lane (tools/coverage_map.py: 30+ rows 15-30 % here against 26-48 % there; 17-24 rows
        // only while several requests share a wave)
        // ... unless the Piola map of a vector-valued element on per-request cells fuses here (one pass instead of
        // tabulation + read-modify-write of every table: tools/coverage_map.py --verts --pushforward)
        const bool fuse_small = rq.want_piola && rows % e->sd == 0 && fixed.id < 0 && coop.id < 0 && !coop.fuses && !fixed.fuses &&
                                !(e->sd == 3 && e->n == 2 && order == 2);  // (that instance spills 39 registers)
        if (fuse_small && rows > 24 && order >= 1 && rq.stacked_pio_ok) break;
        // (36 rows of degree-1 tetrahedra -- BDM1, N2 of degree 1 -- stayed generic at 42-46 %: four members, 144 FMAs a table.
        // Second half of round 4, tools/instance_ab.py, 0.8 GB, generic -> lane-local: BDM2 / N2 triangles with Hessians at 6 / 12
        // points 306 / 251 -> 188 / 188 us (with cells 319 / 260 -> 188 / 188), BDM1 tetrahedra values / gradients at 4 points
        // 159 / 216 -> 141 / 169, at 11 points 231 -> 177; with Hessians the ten tables of 36 rows are slower here, 209 -> 350: not taken)
        const int row_cap = (e->sd == 3 && e->n == 1 && order <= 1) ? 36 : 24;
        if (fuse_small ? rows > 36 : !values_only_shape && (rows > row_cap || (rows > 16 && P == 1))) break;
        out.id = (int)i;
        out.fuses = fuse_small;
        out.P = P;
        break;
    }
    return out;
}

// ---- stacked-matrix kernel (requests on the element's own cell, large shapes)? ------------------------------------------------
// the kinds of a row (StackedShape::rtc)
constexpr bool row_inmix(const StackedShape& k) { return k.rtc == -2 || k.rtc == -3 || k.rtc == -4 || k.rtc == -5 || k.rtc == -6; }  // chain rule / Piola map inside the kernel
constexpr bool row_chunked(const StackedShape& k) { return k.rtc == -1 || k.rtc == -4 || k.rtc == -5; }
constexpr bool row_wg(const StackedShape& k) { return k.rtc == -7; }

// among the instances of one kind that hold the request, the one with the fewest padding columns
bool tighter_instance(const StackedShape& k, int npts) {
    for (const StackedShape& o : kStackedShapes)
        if (o.sd == k.sd && o.n == k.n && o.rtc == k.rtc && 16 * o.ct / o.g >= npts &&
            (16 * o.ct / o.g < 16 * k.ct / k.g || (16 * o.ct / o.g == 16 * k.ct / k.g && o.ct < k.ct)))
            return true;
    return false;
}

// is there a whole-request instance of four column tiles for the row's (sd, n)?
bool has_whole_four_tiles(const StackedShape& k) {
    for (const StackedShape& o : kStackedShapes)
        if (o.sd == k.sd && o.n == k.n && o.rtc == 0 && o.g == 1 && o.ct == 4) return true;
    return false;
}

// the per-wave kernel has an 8-byte twin for the odd tables of this (sd, n) at `npts`: degree-3 / -4 tetrahedra up to 24
// points, degree-5 triangles from 25 points up to `tri5_last` (the whole-request twin ends at 32, the chain-rule twin at 48)
bool per_wave_odd_twin(const StackedShape& k, int npts, int tri5_last) {
    return (k.sd == 3 && (k.n == 3 || k.n == 4) && npts <= 24) || (k.sd == 2 && k.n == 5 && npts >= 25 && npts <= tri5_last);
}

// (first the instances that apply the chain rule themselves, then the rest, each in table order)
// the request-per-workgroup kernel applies the order-1 chain rule of per-request cells itself (round 4, MIX instances):
// rules of 49..128 points, the window of P5 triangles, or policy wg_small -- the per-wave chain-rule instances yield
bool wg_mix_takes(const StackedShape& k, const Request& rq) {
    const fx_element* e = rq.e;
    const int rows = rq.rows, npts = rq.npts;
    if (rq.has(FX_POLICY_NO_WG | FX_POLICY_NO_STACKED_MIX) || !rq.has_cells || rq.order != 1 || npts > 128) return false;
    // (49..64 points, two requests per slab: tools/instance_ab.py [--policy wg_small], sustained, 0.8 GB -- N3 / RT3 tetrahedra at
    // 57 / 50 points 315 / 316 -> 199 / 190 us, P3 / P4 / P5 / P6 at 57 points 384 / 412 / 464 / 544 -> 279 / 328 / 333 / 434, P6
    // triangles at 49 / 60 points 427 / 394 -> 302 / 253, P5 at 55 points 515 -> 313: the former routes were a second
    // 48-point chunk that is mostly padding, or a four-tile whole-request instance plus the table-mixing pass)
    // (... and two windows the off-default audits found, tools/coverage_map.py --audit --verts --qdeg-offset -1, confirmed in
    // sustained runs: vector-valued degree-3 tetrahedra at 13..15 points -- N3 / RT3 / BDM3 at the 14-point rule 407 / 352 / 374 ->
    // 229 / 174 / 181 us, nine requests per slab against the three-request instance + table-mixing pass -- and tables of an odd
    // number of doubles at 17..48 points, which only the point chunks or a whole-request instance + mixing pass held: P5
    // triangles at 19 points 589 -> 307 us, P4 tetrahedra at 31 points 401 -> 314)
    // (where the per-wave kernel has an 8-byte twin of its chain-rule instance it keeps the odd tables: N3 tetrahedra at the
    // 23-point rule 198 us there against 213 here)
    const bool odd_pt = ((long long)rows * npts) % 2 != 0;
    const bool twin2 = per_wave_odd_twin(k, npts, 48);  // (only read at <= 48 points)
    const bool window = npts > 48 || (k.sd == 2 && k.n == 5 && npts >= 25 && npts <= 33) ||
                        (k.sd == 3 && k.n == 3 && e->vdim > 1 && npts >= 13 && npts <= 15) ||
                        // (degree >= 4 tetrahedra at 13..15 points, nine requests per slab: P4 / P5 / P6 at 14 points 403 / 485 / 580 ->
                        // 272 / 292 / 393 us)
                        (k.sd == 3 && k.n >= 4 && npts >= 13 && npts <= 15) ||
                        (odd_pt && npts >= 17 && npts <= 48 && !twin2);
    if (!(window || rq.has(FX_POLICY_WG_SMALL))) return false;
    const int g = npts > 64 ? 1 : std::min(12, 128 / npts);
    const int ctn = std::max(4, (g * npts + 15) / 16);
    const int ctm = fxwg::mix_ct(k.sd, k.n, ctn);
    if (ctm == 0) return false;
    // (two waves per row tile work on two dof tiles at a time: with few rows the second pair multiplies padding -- P3 / P4
    // tetrahedra at 70 / 74 points 424 / 406 us against 388 / 403 us on the point chunks -- so at least 70 % of those
    // MFMA rows must be dofs; the eight-tile instances of tetrahedra, and of triangles with odd tables, run all four waves on one dof tile)
    const bool oddm = odd_tables(rows, npts);
    if (!(ctm == 8 && (k.sd == 3 || oddm))) {   // (wg.hip wg_mix_pc: those instances run four waves per dof tile)
        const int rtd = (rows + 15) / 16;
        if (10LL * rows < 7LL * 16 * 2 * ((rtd + 1) / 2)) return false;
    }
    return fxwg::has_mix_instance(k.sd, k.n, ctm, oddm) && fxwg::lds_bytes(k.sd, k.n, ctm) <= rq.lds_per_cu;
}

// what the stacked stage reads of the stages before it
struct StackedGate {
    bool small_chosen;       // the lane-local kernel holds the request ...
    bool small_values_only;  // ... on one of its values-only rows
    bool small_keeps;        // ... and keeps it unless an in-kernel chain-rule row (rtc -2 / -3) takes it
    bool stacked_small;      // policy: the register-resident rows are open
    long long min_rows;      // FIAT_AMD_STACKED_MIN_ROWS
};

// what every kind of row has to pass first
bool row_open(const StackedShape& k, const Request& rq, const StackedGate& gate) {
    const fx_element* e = rq.e;
    const int order = rq.order, npts = rq.npts;
    const bool verts = rq.has_cells, inmix = row_inmix(k);
    if (gate.small_keeps && k.rtc != -3 && k.rtc != -2) return false;
    if (k.sd != e->sd || k.n != e->n) return false;
    // small shapes with register-resident fragments: A/B partner of the paired kernel only (measured
    // equal on C2, 302 vs 303 us -- both sit on the store-path plateau -- and the paired kernel's
    // recurrence derivatives are two digits more accurate), opt-in with FIAT_AMD_STACKED_SMALL=1
    if (k.rtc > 0 ? (rq.RT != k.rtc || verts || !gate.stacked_small) : (rq.R < gate.min_rows || (rq.R < 16 && gate.small_chosen))) return false;
    // (per-request cells with derivatives on the low-degree shapes: the second pass over the tables costs more
    // than the generic kernel's in-kernel chain rule -- tools/small_vs_stacked.py --verts, 18-29 % against 25-48 %)
    if (!inmix && verts && order >= 1 && (k.n <= 2 || (k.sd == 2 && k.n <= 4))) return false;
    // (the same for vector-valued degree-3 tetrahedra at up to 16 points, round 3 audit: N3 / RT3 / BDM3 with Hessians at
    // 11 / 16 points 525 / 450, 447 / 425, 492 / 461 us on the three-request instance plus mixing pass against 404 / 312,
    // 375 / 288, 426 / 312 us generic; N3 with gradients 392 / 324 against 338 / 221, but 379 against 398-444 at 14 points: kept there)
    if (!inmix && verts && k.sd == 3 && k.n == 3 && e->vdim > 1 && (order == 2 ? npts <= 16 : order == 1 && (npts <= 12 || npts == 16))) return false;
    // (own cell, gradients of P3 / P4 triangles where the lane-local kernel holds the request -- round 3, ABAB with
    // tools/instance_ab.py --own-cell [--policy no_stacked]: P3 at 6 / 7 / 10 / 15 / 25 points 195 / 197 / 172 / 170 / 199 us
    // here against 149 / 149 / 144 / 157 / 149 us lane-local, while 8 / 12 / 16 / 24 points are level or better here;
    // P4 at odd sizes up to 16 points falls to the point-chunked instance, 407 us against 264 us at 15 points)
    if (!verts && order == 1 && gate.small_chosen && k.sd == 2 &&
        ((k.n == 3 && npts % 8 != 0 && npts != 12) || (k.n == 4 && k.rtc == -1 && npts <= 16)))
        return false;
    // (values-only P5 triangles where the lane-local kernel holds several requests per wave: round 4)
    if (order == 0 && gate.small_values_only) return false;
    return true;
}

// rtc -2 / -3 / -6 -- per-request cells, order 1 / 2: chain rule across the tables inside the kernel (dof-major tiles)
bool takes_inkernel(const StackedShape& k, const Request& rq, bool& pio, bool& mix_odd) {
    const int npts = rq.npts;
    if (rq.has(FX_POLICY_NO_STACKED_MIX) || !rq.has_cells || rq.order != (k.rtc == -2 ? 1 : k.rtc == -3 ? 2 : 0)) return false;
    if (k.rtc == -2 && wg_mix_takes(k, rq)) return false;
    // the element's Piola map too (vector-valued elements: the twin with the components of a dof in one lane,
    // 12 rows per tile in 3-D); values only: nothing else to mix, so only with the map
    pio = rq.want_piola && k.pio && (rq.pio_even || (rq.pio_odd_twin && k.pio_odd));
    if (k.rtc == -6 && !pio) return false;
    // (16-byte pieces of whole tables; the rows with an 8-byte twin take odd table sizes too: P5 triangles at the
    // 25-point rule, N3 and RT2 tetrahedra at the 23- and 11-point rules; off-default rules of odd size: P4
    // tetrahedra at 17-24 points (the 23-point rule), P4 triangles at 25-32, P5 triangles at 33-48 (the 33-point rule))
    mix_odd = odd_tables(rq.rows, npts);
    // (RT2 at order 1 stays on the generic kernel: 44.7 % of the HBM peak there, 39.2 % on the twin)
    if (pio) mix_odd = !rq.pio_even;
    if (mix_odd && !pio && !k.odd) return false;
    return holds_request(k, npts) && !tighter_instance(k, npts) && fills_tiles(k, npts);
}

// rtc -7 -- a request (or a group of small requests) per workgroup
bool takes_workgroup(const StackedShape& k, const Request& rq, WgFacts& wg) {
    const fx_element* e = rq.e;
    const int order = rq.order, rows = rq.rows, npts = rq.npts, RT = rq.RT;
    const bool verts = rq.has_cells, even = rq.even;
    if (rq.has(FX_POLICY_NO_WG) || npts > 16 * k.ct) return false;
    // (fewer than 49 points: the whole-request instances of the per-wave kernel -- except where several requests per
    // workgroup are robustly ahead in sustained runs, tools/instance_ab.py --own-cell [--policy wg_small], 0.8 GB:
    // P5 triangles with derivatives at 25..33 points 232 / 183 / 252 -> 189 / 169 / 225 us, degree-6 tetrahedra with
    // Hessians at 33..48 points 432 -> 352 us.  Elsewhere the two are within +-10 % of each other with either sign,
    // and the map's short interleaved runs disagree with the sustained ones: opt-in, policy wg_small)
    // (vector-valued degree-3 tetrahedra of 180 rows a table -- BDM3, N2 of degree 3 -- at 17..24 points with cells, values:
    // 892 -> 744 us at the 23-point rule in 4 GB batches.  What the 0.8 GB runs of the audits showed beside it -- their
    // other orders, 13..15 points on the own cell, 49..64 points with derivatives -- is within +-4 % at 4 GB: not taken)
    // (... and on the own cell: 904 -> 742 us; gradients / Hessians there 1.07 / 1.01, RT3 / N3 values 0.91 / 1.10: not taken)
    const bool vec3_rows = k.sd == 3 && k.n == 3 && e->vdim > 1 && rows >= 160;
    // (after the kernel's second half of round 4, sustained default / wg_small sweep over 135 shapes, own cell and cells:
    // degree >= 5 tetrahedra at 13..15 points, nine requests per slab -- P5 / P6 at 14 points, values / gradients / Hessians
    // 352 / 272 / 302 -> 316 / 237 / 236 us and 465 / 371 / 439 -> 401 / 328 / 314, with cells 368 / - / 571 -> 351 / - / 472 and
    // 477 / - / 697 -> 422 / - / 549; P4 with Hessians 208 -> 187, with cells 477 -> 438; values of degree >= 5 at 25..32
    // points, four per slab, 363 / 466 -> 319 / 410.  Confirmed in 4 GB batches (CAP_GB=4): 0.91-0.97 of the per-wave
    // instances there, 0.89 / 0.91 at 25..32 points -- while P6 with Hessians at the 23-point rule, 438 -> 366 us at 0.8 GB,
    // is 1.04 at 4 GB and 7.51 against 6.93 ms in bench.py --workload dg6tet: heavy requests are few at 0.8 GB and the
    // two kernels quantise differently over the chip; windows are taken from the larger batches)
    const bool hi14 = k.sd == 3 && npts >= 13 && npts <= 15 && (k.n >= 5 || (k.n == 4 && order == 2));
    const bool hi_more = k.sd == 3 && k.n >= 5 && order == 0 && npts >= 25 && npts <= 32;
    const bool small_window = (k.sd == 2 && k.n == 5 && order >= 1 && npts >= 25 && npts <= 33) ||
                              (k.sd == 3 && k.n == 6 && order == 2 && npts >= 33 && npts <= 48) || hi14 || (hi_more && !verts);
    // per-request cells with gradients: the chain rule on the accumulators (MIX instances); other orders with
    // cells: values straight from the kernel, derivatives + the table-mixing pass
    const bool want_mix = verts && order == 1 && !rq.has(FX_POLICY_NO_STACKED_MIX);
    // (tables of an odd number of doubles at 17..48 points had only the point chunks: P5 triangles with gradients at 19
    // points 361 -> 201 us, values of P4 tetrahedra at 31 points 515 -> 394; with cells 586 -> 459)
    // (not where a whole-request instance has an 8-byte twin: values of P4 tetrahedra at the 23-point rule 315 us there,
    // 422 here)
    const bool twin1 = per_wave_odd_twin(k, npts, 32);
    const bool odd_window = !even && npts >= 17 && npts <= 48 && (!verts || order == 0) && !twin1;
    if (npts <= 48 && !rq.has(FX_POLICY_WG_SMALL) && !(small_window && (!verts || want_mix)) && !odd_window &&
        !(order == 0 && vec3_rows && npts >= 17 && npts <= 24) &&
        !(verts && order != 1 && (hi14 || hi_more)) &&
        !(want_mix && wg_mix_takes(k, rq)))
        return false;
    // requests per slab of <= 128 columns and the instance's column tiles
    wg.g = npts > 64 ? 1 : std::min(12, 128 / npts);
    wg.ct = std::max(4, (wg.g * npts + 15) / 16);
    if (want_mix) {
        // (tetrahedra: 4 column tiles with two waves per row tile or 8 with four; triangles 4 / 6 / 8 with two)
        wg.ct = fxwg::mix_ct(k.sd, k.n, wg.ct);
        wg.odd = odd_tables(rows, npts);
        wg.mix = wg.ct > 0 && fxwg::has_mix_instance(k.sd, k.n, wg.ct, wg.odd) && wg_mix_takes(k, rq);
    }
    if (!wg.mix) {
        if (verts && order >= 1 && npts <= 48 && !rq.has(FX_POLICY_WG_SMALL) && !(hi14 && order == 2)) return false;
        // (65..96 points -- five or six column tiles -- with a short K loop: a stage is a few dozen MFMAs and the
        // per-request recurrence + barriers dominate.  tools/instance_ab.py --own-cell [--policy no_wg], 0.8 GB, this
        // kernel against the point chunks: P4 tetrahedra at 70 points, values / gradients 779 / 435 against 455 / 270 us,
        // P3 528 / 232 against 345 / 217, P5 triangles at 79 points 556 / 358 against 334 / 234, P6 triangles values
        // 455 against 320 -- while degree >= 5 tetrahedra (K steps >= 14) and P6 triangles with Hessians win, as does
        // everything at 97..128 points.  Policy wg_small opts in regardless.)
        wg.odd = !even;
        wg.ct = std::max(4, (wg.g * npts + 15) / 16);
        if (wg.ct == 7) wg.ct = 8;        // (no seven-tile instance)
        if (wg.ct == 5) {                  // one wave per row tile on 5 column tiles, or two on 3 + 3: the fewer MFMA slots per wave
            const long long one = (long long)((RT + 3) / 4) * 5, two = (long long)((RT + 1) / 2) * 3;
            // (the one-wave-per-row-tile layout holds ONE request per slab: twelve requests of 6 points -- policy
            // wg_small, 72 columns -- were planned onto it and refused by the launch, hipErrorInvalidValue)
            if (two < one || wg.g > 1) wg.ct = 6;
        }
        // (... except the instances of one wave per row tile on five column tiles, since the recurrence coefficients are
        // fetched ahead and the last tile of a group leaves under the next group's MFMAs (second half of round 4;
        // sustained, same tool): values of P4 tetrahedra at 74 / 75 points 358 / 394 us against 432 / 429 on the point
        // chunks, RT3 values / P3 Hessians at 74 points 175 / 164 against 202 / 197, P5 triangles with gradients at 65 / 72 /
        // 79 points 240 / 187 / 224 against 261 / 240 / 235 -- while two waves per row tile on six column tiles still lose
        // with few rows: P6 triangles, values at 79 points 359 against 296, P3 tetrahedra at 70 points 460 against 348)
        if (npts > 64 && (wg.g * npts + 15) / 16 <= 6 && !rq.has(FX_POLICY_WG_SMALL) &&
            !((e->nexp + 3) / 4 >= 14 || (k.sd == 2 && k.n == 6 && order == 2) || wg.ct == 5))
            return false;
        if (!fxwg::has_instance(k.sd, k.n, wg.ct, wg.odd)) return false;
    }
    // (49..64 points: where a whole-request instance of four column tiles exists it keeps the rule)
    // (... except degree >= 5 tetrahedra: two requests per slab 0.87-0.93 of the four-tile instance at 57 points)
    if (!wg.mix && npts > 48 && npts <= 64 && even && !rq.has(FX_POLICY_WG_SMALL) && !(k.sd == 3 && k.n >= 5) && has_whole_four_tiles(k))
        return false;
    return rq.nreq + 3LL * rq.num_cu <= 0x7fffffffLL;
}

// rtc -1 / -4 / -5 -- point-chunked: whatever the whole-request instances above did not take
bool takes_chunks(const StackedShape& k, const Request& rq) {
    const int order = rq.order, npts = rq.npts;
    if (npts < 13 || rq.nreq * (long long)((npts + 16 * k.ct - 1) / (16 * k.ct)) > 0x7fffffffLL) return false;
    if ((k.rtc == -1 || k.rtc == -4) && k.sd == 3 && (k.n == 6 || k.n == 5)) {
        // two-tile or three-tile chunks: the fewer column tiles.  Measured (tools/instance_ab.py --own-cell, 0.8 GB): degree 6
        // at the 122-point rule, values / gradients / Hessians 581 / 469 / 540 us on 48-point chunks (9 tiles) -> 535 / 364 /
        // 353 us on 32-point chunks (8 tiles); at 57 points (6 -> 4 tiles) gradients 426 us.  On a tie (74 points: 6 tiles
        // either way) degree 6 is faster on 48-point chunks (402 against 448 us) and degree 5 within the spread of the two
        // measurement protocols (361-370 us in sustained runs, 410-428 in the map's short ones, against 385-400): ties stay
        // on 48-point chunks
        const long long t2 = 2LL * ((npts + 31) / 32), t3 = 3LL * ((npts + 47) / 48);
        if ((k.ct == 2) != (t2 < t3)) return false;
    }
    if (row_inmix(k)) {  // ... with the chain rule inside: rules of more than one chunk
        if (rq.has(FX_POLICY_NO_STACKED_MIX) || !rq.has_cells || order != (k.rtc == -4 ? 1 : 2) || npts <= 16 * k.ct) return false;
        if (k.rtc == -4 && wg_mix_takes(k, rq)) return false;
        // (49..64 points: the second chunk of 48 is mostly padding.  Round 3 audit, ABAB tools/instance_ab.py
        // [--policy no_stacked_mix]: where a whole-request instance of four column tiles exists and the stacked
        // matrix is small, that instance plus the mixing pass is faster -- gradients of P3 / P4 / P5 tetrahedra at
        // 50 points 532 / 557 / 614 -> 392 / 428 / 516 us, P5 / P6 triangles 567 / 479 -> 421 / 423 us, Hessians of P3
        // tetrahedra and P5 triangles 512 / 513 -> 411 / 424 us; from ~250 stacked rows on the pass over the tables
        // costs more than the padding: N3 tetrahedra 318 against 395 us, Hessians of P4 / P5 tetrahedra 397 / 446
        // against 467 / 539 us, and of P6 triangles at 168 rows 397 against 426 us)
        if (npts <= 64 && rq.even && rq.R <= 224 && !(order == 2 && k.sd == 2 && k.n == 6) && has_whole_four_tiles(k)) return false;
    }
    return true;
}

// rtc 0 and the register-resident rows (rtc > 0) -- whole requests
bool takes_whole(const StackedShape& k, const Request& rq) {
    // (16-byte stores of whole request chunks; a few instances have an 8-byte twin for odd request sizes)
    // (with per-request cells the 8-byte twin works as it is: the cells only enter the production phase, and the
    // chain rule across the tables is the separate mixing pass -- P5 triangles at the 25-point rule with cells ran on
    // the point-chunked instance at 17.6 % against 27-37 % on their own cell)
    // KEPT AS FOUND (DESIGN.md 10.1a, to be fixed on its own): a register-resident row (rtc > 0) has no 8-byte twin,
    // but the former hand list went by (sd, n, ct, g) and so let it pass wherever its whole-request sibling has
    // one -- <3, 3, 3, 2, 5>, policy stacked_small, order 0, an odd number of 65..79 rows.  L.kodd stays false for
    // rtc > 0, so run_stacked launches the row's 16-byte base instance on those odd tables, as it always did.
    if (!rq.even && !k.odd) {
        bool sibling_odd = false;
        for (const StackedShape& o : kStackedShapes)
            sibling_odd = sibling_odd || (k.rtc > 0 && o.rtc == 0 && o.odd && o.sd == k.sd && o.n == k.n && o.ct == k.ct && o.g == k.g);
        if (!sibling_odd) return false;
    }
    return holds_request(k, rq.npts) && !tighter_instance(k, rq.npts) && fills_tiles(k, rq.npts);
}

// `fused`: an earlier stage applies the Piola map.  Builds the element's stacked matrix (ensure_stacked, device work) for the
// first row whose predicates pass; a row that the matrix, the cell or the CU's LDS then refuse is skipped, the next one tried.
int choose_stacked(const Request& rq, const FixedChoice& fixed, const SmallChoice& small, bool fused, StackedChoice& out) {
    const fx_element* e = rq.e;
    const int order = rq.order, npts = rq.npts;
    const bool verts = rq.has_cells;
    // (fewer stacked rows: the production of the B fragments is no longer amortised over enough row tiles)
    // (measured, tools/coverage_map.py: values-only requests of P3 / P4 tetrahedra, 20 / 35 rows, run at 45 / 30 % of the HBM
    // peak here against 23 / 13 % on the generic kernel; below one row tile nothing is left to amortise)
    // (15 rows: values-only P4 triangles 27-30 % lane-local -> 38-49 % here; 10 rows -- P3 triangles, P2 tetrahedra -- stay
    // lane-local, 39-43 % against 34-39 %)
    // (round 3, tools/coverage_map.py --audit: since the lane-local kernel packs several requests per lane group it serves
    // the 15-row tables faster wherever it holds them -- 6 / 16 / 25 / 32 points: 165 / 157 / 211 / 157 us against
    // 249 / 191 / 412 / 282 us here -- so below one full row tile this kernel only takes what the lane-local one refuses)
    static const long long stacked_min_rows = ab_env("FIAT_AMD_STACKED_MIN_ROWS") ? atoll(ab_env("FIAT_AMD_STACKED_MIN_ROWS")) : 15;
    // (after the shape-specialised registries: the tuned paired instances and the lane-local kernel keep their shapes)
    // (per-request cells: the kernel maps the points through the request's cell and a second pass applies the
    // chain rule across the derivative tables, table_mix_kernel; a Piola map is left to fx_pushforward_batch)
    // (the lane-local kernel keeps the shapes no stacked instance takes -- degrees 1 and 2 on triangles, degree 1 on
    // tetrahedra, fewer than 16 stacked rows -- and per-request cells, where it applies the chain rule itself; elsewhere
    // the MFMA contraction wins: tools/coverage_map.py, P3 / P4 triangles and P2 tetrahedra with derivatives 26-52 % -> 50-69 %)
    // (order 2 with per-request cells: the rtc -3 instances beat the lane-local kernel on P4 triangles and P2 tetrahedra,
    // 21 -> 58 % and 19 -> 38 % of the HBM peak, tools/coverage_map.py --verts --order 2 [--policy no_small])
    const bool small_keeps = small.id >= 0 && verts;
    // (round 3 audit, ABAB with tools/instance_ab.py [--policy no_small]: gradients of P4 triangles 264 / 213 / 260 / 293 / 218 us
    // lane-local at 12 / 16 / 24 / 25 / 32 points against 193 / 164 / 162 / 259 / 164 us on the rtc -2 instances; Hessians of P3
    // triangles at 15 / 16 points 280 / 259 against 216 / 202 us -- level or behind at the other sizes; P3 triangles and P2
    // tetrahedra with gradients stay lane-local, 151-220 against 177-262 us)
    const bool over_small = (order == 2 && ((e->sd == 2 && e->n >= 4) || (e->sd == 3 && e->n >= 2) ||
                                            (e->sd == 2 && e->n == 3 && npts >= 13 && npts <= 16))) ||
                            (order == 1 && e->sd == 2 && e->n == 4);
    // (round 3, tools/coverage_map.py --audit + tools/instance_ab.py --own-cell, ABAB at 1.5 GB of tables: on the element's own
    // cell the stacked kernel now beats the paired instances of P3 tetrahedra with gradients outside the 21..24-point
    // benchmark shape -- 12 / 14 / 28 / 32 / 44 points: 294 / 296 / 304 / 282 / 284 us paired, 270 / 256 / 259 / 249 / 257 us
    // here -- and of P4 tetrahedra, 400 / 373 us -> 316 / 303 us at 22 / 24 points; with per-request cells the paired kernel
    // applies the chain rule on its accumulators and keeps every shape, 285-345 us against 365-750 us.  Those entries yield
    // when an instance here holds the request.)
    const bool fixed_yields = fixed.id >= 0 && !verts && !fused && order == 1 && e->sd == 3 &&
                              ((e->n == 3 && kFixedShapes[fixed.id].nt != 6) || e->n == 4);
    if (rq.has(FX_POLICY_NO_STACKED) || !(fixed.id < 0 || fixed_yields) || !(!small_keeps || over_small) || fused || e->raw_expansion || order > 2)
        return FX_OK;
    const StackedGate gate{small.id >= 0, small.id >= 0 && kSmallShapes[small.id].values_only, small_keeps,
                           rq.has(FX_POLICY_STACKED_SMALL), stacked_min_rows};
    // (first the instances that apply the chain rule themselves, then the request-per-workgroup instances, then the rest,
    // each in table order)
    for (unsigned pass = 0; pass < 3; ++pass)
        for (int i = 0; i < NSTACKED; ++i) {
            const StackedShape& k = kStackedShapes[i];
            const bool inmix = row_inmix(k), chunked = row_chunked(k), wgk = row_wg(k);
            if (pass != (inmix ? 0u : wgk ? 1u : 2u)) continue;
            if (!row_open(k, rq, gate)) continue;
            bool pio = false, mix_odd = false;
            WgFacts wg;
            const bool takes = (k.rtc == -2 || k.rtc == -3 || k.rtc == -6) ? takes_inkernel(k, rq, pio, mix_odd)
                               : wgk                                       ? takes_workgroup(k, rq, wg)
                               : chunked                                   ? takes_chunks(k, rq)
                                                                           : takes_whole(k, rq);
            if (!takes) continue;
            if (!k.matches(e->prog)) continue;
            int rc = ensure_stacked(rq.ctx, const_cast<fx_element*>(e), order);
            if (rc != FX_OK) return rc;
            if (e->stack_state[order] != 1) continue;
            const bool dofmajor = inmix || wg.mix;
            const double* afrag = pio ? e->d_astack_dmp[order].get() : dofmajor ? e->d_astack_dm[order].get() : e->d_astack[order].get();
            if (!afrag) continue;
            if (dofmajor && !invert_small(e->sd, e->A0, out.A0inv)) continue;
            const bool mixr = pio || mix_odd || k.mixr;  // of the twin run_stacked will take
            const int slots = fxk::stacked_mix_slots(e->sd, dofmajor ? rq.ntab : 0, mixr);
            int lds_bytes = (fxk::WQ_CTL_DOUBLES + STACKED_NW * (fxk::stacked_image_doubles(k.ct, (e->nexp + 3) / 4, slots) + (mixr ? fxk::STACKED_KBUF : 0))) * 8;
            if (wgk) lds_bytes = fxwg::lds_bytes(k.sd, k.n, wg.ct);
            if (lds_bytes > rq.lds_per_cu) continue;
            const long long groups = wgk ? ((rq.nreq + wg.g - 1) / wg.g) * STACKED_NW : chunked ? rq.nreq * ((npts + 16 * k.ct - 1) / (16 * k.ct)) : (rq.nreq + k.g - 1) / k.g;
            // one workgroup per CU = one wave per SIMD (measured: a second wave per SIMD at half the registers
            // spills in the production phase and gains nothing, 1.45 -> 1.48 ms: the kernel is bound by the
            // shared fp64 MFMA/VALU pipe, not by latencies)
            // (the request-per-workgroup kernel's one-row-tile instances -- values-only requests of up to 64 rows -- are the
            // exception: 256 registers, two workgroups a CU, 320 -> 298 us for degree-5 tetrahedra at 74 points)
            const int wgs = wgk ? fxwg::workgroups_per_cu(k.sd, k.n, wg.ct, wg.odd, wg.mix ? 1 : 0, rq.RT) : 1;
            out.id = i;
            out.pio = pio;
            out.mix_odd = mix_odd;
            out.kodd = wgk ? wg.odd : ((k.rtc == 0 && !rq.even) || mix_odd);
            out.dofmajor = dofmajor;
            out.wg = wg;
            out.afrag = afrag;
            out.lds_bytes = lds_bytes;
            out.grid = (int)std::max<long long>(1, std::min<long long>((groups + STACKED_NW - 1) / STACKED_NW, (long long)rq.num_cu * wgs));
            out.fixed_yields = fixed_yields;
            return FX_OK;
        }
    return FX_OK;
}

// ---- filling: the winner's argument struct and Launch fields ----------------------------------------------------------------
// what the five argument structs have in common
template <class Args>
void fill_header(Args& a, const Request& rq, const double* pts, const double* verts, double* out) {
    memset(&a, 0, sizeof a);
    a.pts = pts;
    a.verts = verts;
    a.out = out;
    a.phi0 = rq.e->prog.phi0;
    memcpy(a.A0, rq.e->A0, sizeof a.A0);
    memcpy(a.b0, rq.e->b0, sizeof a.b0);
    a.nreq = rq.nreq;
    a.npts = rq.npts;
}
// A, B, C of every recurrence step
void copy_abc(const fx::Program& prog, double* dst) {
    for (size_t k = 0; k < prog.steps.size(); ++k) {
        dst[3 * k + 0] = prog.steps[k].A;
        dst[3 * k + 1] = prog.steps[k].B;
        dst[3 * k + 2] = prog.steps[k].C;
    }
}

void fill_generic(Launch& L, const Request& rq, const GenericShape& g, const double* pts, const double* verts, double* out) {
    const fx_element* e = rq.e;
    fxk::TabArgs& a = L.args;
    fill_header(a, rq, pts, verts, out);
    a.afrag = e->d_afrag.get();
    a.steps = e->d_steps.get();
    a.rows = rq.rows;
    a.nexp = e->nexp;
    a.nsteps = (int)e->prog.steps.size();
    a.KS = e->KS;
    a.MT = e->MT;
    a.ntab = rq.ntab;
    a.debug = rq.debug;
    a.P = g.P;
    a.pc = g.pc;
    a.nchunk = g.nchunk;
    a.nitems = g.nitems;
    a.phi_doubles = g.phi_doubles;
    a.stage_doubles = g.stage_doubles;
    L.lds_bytes = g.lds_bytes;
    int per_cu = std::max(1, std::min(16, rq.lds_per_cu / std::max(1, L.lds_bytes)));
    long long want = (long long)rq.num_cu * per_cu * 4;
    L.grid = (int)std::max<long long>(1, std::min<long long>(a.nitems, want));
}

void fill_coop(Launch& L, const Request& rq, const CoopChoice& c, const double* pts, const double* verts, double* out) {
    const fx_element* e = rq.e;
    fxk::CoopArgs& ca = L.cargs;
    fill_header(ca, rq, pts, verts, out);
    ca.afrag = e->d_afrag_coop.get();
    ca.eint = e->d_coop_eint.get();
    ca.edbl = e->d_coop_edbl.get();
    ca.kstart = e->d_coop_kstart.get();
    ca.rows = rq.rows;
    ca.KS = e->coop_KS;
    ca.NT = c.nt_need;
    ca.emax = e->coop_emax;
    ca.TR = c.TR;
    ca.slab_doubles = c.nt_need * 64 + 128;
    ca.img_doubles = c.img_doubles;
    ca.debug = rq.debug;
    ca.piola = c.fuses ? rq.mapping : 0;
    if (c.fuses) memcpy(ca.A0inv, c.A0inv, sizeof ca.A0inv);
    L.clds_bytes = c.lds_bytes;
    int per_cu = std::max(1, std::min(2, rq.lds_per_cu / L.clds_bytes));
    L.cgrid = (int)std::max<long long>(1, std::min<long long>(rq.nreq, (long long)rq.num_cu * per_cu));
}

void fill_fixed(Launch& L, const Request& rq, const FixedChoice& f, const double* pts, const double* verts, double* out) {
    const fx_element* e = rq.e;
    fxk::FixedArgs<0>& fa = L.fhead;
    fill_header(fa, rq, pts, verts, out);
    L.fcoef.resize(e->prog.steps.size() * 3);
    L.fucoef.assign(e->prog.steps.size() * 12, 0.0);
    copy_abc(e->prog, L.fcoef.data());
    for (size_t k = 0; k < e->prog.steps.size(); ++k) {
        const fx::Step& st = e->prog.steps[k];
        // point-independent derivatives of the collapsed-coordinate factors on the
        // element's own cell (rows of A0 padded with zeros, expansions.py:43-63)
        const int sd = e->sd;
        double dfa[3] = {0, 0, 0}, dfb[3] = {0, 0, 0};
        for (int d = 0; d < sd; ++d) {
            double dx = e->A0[st.codim * sd + d];
            double dy = st.codim + 1 < sd ? e->A0[(st.codim + 1) * sd + d] : 0.0;
            double dz = st.codim + 2 < sd ? e->A0[(st.codim + 2) * sd + d] : 0.0;
            dfb[d] = 0.5 * (dy + dz);
            dfa[d] = dx + dfb[d];
        }
        double* u = &L.fucoef[12 * k];
        for (int d = 0; d < sd; ++d) {
            u[d] = st.A * dfa[d] - st.B * dfb[d];
            u[3 + d] = -2.0 * st.C * dfb[d];
        }
        int h = 0;
        for (int d1 = 0; d1 < sd; ++d1)
            for (int d2 = d1; d2 < sd; ++d2) u[6 + h++] = -2.0 * st.C * dfb[d1] * dfb[d2];
    }
    L.fkind = f.fkind;
    L.ncu = rq.num_cu;
    L.trash = rq.ctx->d_trash.get();
    L.ctx = rq.ctx;   // (the paired kernel draws its work counter at the launch, when the stream is known: work_counter)
    fa.afrag = f.fkind >= 1 ? e->d_afrag_stream.get() : e->d_afrag_split.get();
    fa.debug = (rq.debug & 0xffff) | (f.fuses ? (rq.mapping << 16) : 0);
    fa.lds_doubles = f.lds_doubles;
    L.flds_bytes = f.lds_bytes;
    L.fgrid = f.grid;
}

void fill_small(Launch& L, const Request& rq, const SmallChoice& s, const double* pts, const double* verts, double* out) {
    const fx_element* e = rq.e;
    fxk::SmallArgs& sa = L.sargs;
    fill_header(sa, rq, pts, verts, out);
    if (s.fuses) {
        sa.piola = rq.mapping;
        for (int q = 0; q < 9; ++q) sa.G[q] = 0.5 * e->A0[q];
    }
    sa.cmat = e->d_cmat.get();
    copy_abc(e->prog, sa.coef);
    sa.nitems = (rq.nreq + s.P - 1) / s.P;
    sa.rows = rq.rows;
    sa.P = s.P;
    sa.stage_doubles = (int)(((long long)s.P * rq.ntab * rq.rows * rq.npts + 1) & ~1LL);
    sa.debug = rq.debug;
    L.slds_bytes = sa.stage_doubles * 8 * SMALL_NW;
    const int wg_per_cu = std::max(1, std::min(8, rq.lds_per_cu / std::max(1, L.slds_bytes)));
    const long long nwg = (sa.nitems + SMALL_NW - 1) / SMALL_NW;
    L.sgrid = (int)std::max<long long>(1, std::min<long long>(nwg, (long long)rq.num_cu * wg_per_cu * 4));
}

void fill_stacked(Launch& L, const Request& rq, const StackedChoice& c, const double* pts, const double* verts, double* out) {
    const fx_element* e = rq.e;
    const StackedShape& k = kStackedShapes[c.id];
    fxk::StackedArgs<0>& ka = L.khead;
    fill_header(ka, rq, pts, verts, out);
    L.fcoef.resize(e->prog.steps.size() * 3);
    copy_abc(e->prog, L.fcoef.data());
    ka.afrag = c.afrag;
    if (c.pio) {
        for (int q = 0; q < 9; ++q) ka.G[q] = 0.5 * e->A0[q];
        ka.piola = rq.mapping;
    }
    if (c.dofmajor) memcpy(ka.A0inv, c.A0inv, sizeof ka.A0inv);
    ka.R = (int)rq.R;
    ka.RT = rq.RT;
    ka.debug = rq.debug;
    ka.lim_pts = (long long)rq.nreq * rq.npts * e->sd;
    ka.lim_verts = verts ? (long long)rq.nreq * (e->sd + 1) * e->sd : 0;
    ka.lim_out = (long long)rq.nreq * rq.R * rq.npts;
    const int TRk = fxk::stacked_tile_rows(e->sd, c.pio ? 1 : 0);
    ka.lim_afrag = (c.dofmajor ? ((long long)((rq.rows + TRk - 1) / TRk) * rq.ntab + 1) : (long long)(rq.RT + 1)) * ((e->nexp + 3) / 4) * 64;
    L.klds_bytes = c.lds_bytes;
    if (row_wg(k)) {
        L.wg_ct = c.wg.ct;
        L.wg_mix = c.wg.mix ? 1 : 0;
        ka.gslab = c.wg.g;
    }
    L.kgrid = c.grid;
    L.ncu = rq.num_cu;
    L.trash = rq.ctx->d_trash.get();
    L.ctx = rq.ctx;
    L.kmix_order = rq.order;
    L.kodd = c.kodd;
    L.kpiola = c.pio ? rq.mapping : 0;
}

// `mapping` != FX_MAP_AFFINE asks for a kernel that fuses the Piola push-forward (L.fused_mapping tells
// whether one was found; otherwise the caller runs fx_pushforward_batch after the launch)
int plan_launch(fx_ctx* ctx, const fx_element* e, int order, int64_t nreq, int npts, const double* pts,
                const double* verts, double* out, Launch& L, int mapping = 0) {
    if (!ctx || !e) return fail(FX_EINVAL, "null context/element");
    if (order < 0) return fail(FX_EINVAL, "negative derivative order");
    if (order > 2) return fail(FX_ENOTIMPL, "derivative order %d > 2 is not implemented on the device", order);
    if (nreq < 0 || npts < 0) return fail(FX_EINVAL, "negative batch size");
    if ((nreq > 0 && npts > 0) && (!pts || !out)) return fail(FX_EINVAL, "null device pointer");
    L.winner = Family::None;
    L.row = -1;
    if (nreq == 0 || npts == 0) return FX_OK;  // empty batch / empty point set: nothing to launch
    const Request rq = make_request(ctx, e, order, nreq, npts, verts != nullptr, mapping);

    // every stage runs, in this order: a later one reads what the earlier ones chose
    GenericShape generic;
    int rc = choose_generic_shape(rq, generic);  // (refuses expansion degrees beyond the LDS tile whichever kernel would take them)
    if (rc != FX_OK) return rc;
    CoopChoice coop;
    rc = choose_coop(rq, coop);
    if (rc != FX_OK) return rc;
    const FixedChoice fixed = choose_fixed(rq, coop);         // (reads: the cooperative kernel fuses the map)
    const SmallChoice small = choose_small(rq, coop, fixed);  // (fuses the map only where neither of the two took the request)
    StackedChoice stacked;
    rc = choose_stacked(rq, fixed, small, coop.fuses || fixed.fuses || small.fuses, stacked);
    if (rc != FX_OK) return rc;

    // the winner: shape-specialised > stacked > cooperative > lane-local > generic; a stacked row supersedes the lane-local
    // choice and, where fixed_yields, the shape-specialised one
    const bool fixed_stays = fixed.id >= 0 && !(stacked.id >= 0 && stacked.fixed_yields);
    if (fixed_stays) {
        L.winner = Family::Fixed, L.row = fixed.id, L.fused_mapping = fixed.fuses;
        fill_fixed(L, rq, fixed, pts, verts, out);
    } else if (stacked.id >= 0) {
        L.winner = Family::Stacked, L.row = stacked.id, L.fused_mapping = stacked.pio;
        fill_stacked(L, rq, stacked, pts, verts, out);
    } else if (coop.id >= 0) {
        L.winner = Family::Coop, L.row = coop.id, L.fused_mapping = coop.fuses;
        fill_coop(L, rq, coop, pts, verts, out);
    } else if (small.id >= 0) {
        L.winner = Family::Small, L.row = small.id, L.fused_mapping = small.fuses;
        fill_small(L, rq, small, pts, verts, out);
    } else {
        L.winner = Family::Generic, L.fused_mapping = false;
        fill_generic(L, rq, generic, pts, verts, out);
    }
    return FX_OK;
}

int run_tabulate(fx_ctx* ctx, const fx_element* e, int order, const Launch& L, hipStream_t s) {
    switch (L.winner) {
        case Family::None: return FX_OK;  // (empty batch / empty point set)
        case Family::Fixed: return run_fixed(L, s);
        case Family::Stacked: return run_stacked(L, s);
        case Family::Coop: return run_coop(L, s);
        case Family::Small: return run_small(order, L, s);
        case Family::Generic: break;
    }
    switch (e->sd) {
        case 1: return launch_sd<1>(order, L, s);
        case 2: return launch_sd<2>(order, L, s);
        case 3: return launch_sd<3>(order, L, s);
    }
    return fail(FX_EINVAL, "Invalid number of spatial dimensions");
}

}  // namespace
