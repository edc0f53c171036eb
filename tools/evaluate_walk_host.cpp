// The per-lane walk of the fused evaluation kernel (fiat_amd/csrc/evaluate.hpp) on the CPU: fold, transform, geometry, walk and
// Piola matrix exactly as the kernel's lanes run them, every compile-time instance (sd, order, vdim), against recorded results.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifiat_amd/csrc tools/evaluate_walk_host.cpp -o walk
//   ./walk cases.txt
//
// cases.txt is written by tests/evaluate_reference.py write_walk_cases from tests/golden/evaluate.npz: per case a header
// "sd n variant order vdim mapping ndof nrhs npts has_verts" and the arrays scale, cell, [verts,] coeffs, dofs, pts,
// ref[ntab(order)][nrhs][vdim][npts], numbers as C hexadecimal floats.  Every case runs at orders 0..order against the leading
// tables of ref.  Exit status 0: every instance ran and stayed within 1e-12 on values and 1e-10 on derivatives in the norm
// max|x - ref| / max(1, max|ref|); 1: a case beyond that; 2: an instance that no case reached, or a malformed file.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "evaluate.hpp"

namespace {

struct Case {
    int sd, n, variant, order, vdim, mapping, ndof, nrhs, npts, has_verts;
    double scale;
    std::vector<double> cell, verts, coeffs, dofs, pts, ref;
};

bool read_doubles(FILE* f, size_t count, std::vector<double>& out) {
    out.resize(count);
    char tok[64];
    for (size_t i = 0; i < count; ++i) {
        if (fscanf(f, "%63s", tok) != 1) return false;
        char* end = nullptr;
        out[i] = strtod(tok, &end);
        if (end == tok || *end) return false;
    }
    return true;
}

// one request at one order: res[ntab][nrhs][vdim][npts]
template <int SD, int ORDER, int VDIM> void run(const Case& c, const fx::EvalTables& t, const std::vector<double>& Ap, std::vector<double>& res) {
    constexpr int NTAB = fxk::eval_binom(SD + ORDER, SD);
    const int vn = VDIM * t.nexp;
    res.assign((size_t)NTAB * c.nrhs * VDIM * c.npts, 0.0);
    double A[SD * SD], b[SD], G[SD * SD];
    fxk::eval_cell_map<SD>(c.cell.data(), A, b);
    for (int i = 0; i < SD * SD; ++i) G[i] = 0.5 * A[i];
    if (c.has_verts) fxk::eval_cell_map<SD>(c.verts.data(), A, b);
    std::vector<double> w((size_t)vn);
    for (int j = 0; j < c.nrhs; ++j) {
        for (int x = 0; x < vn; ++x) {
            double s = 0.0;
            for (int i = 0; i < c.ndof; ++i) s += c.dofs[(size_t)j * c.ndof + i] * Ap[(size_t)i * vn + x];
            w[(size_t)x] = s;
        }
        for (int q = 0; q < c.npts; ++q) {
            fxk::EvalGeom<SD> geo;
            fxk::eval_geom<SD>(A, b, &c.pts[(size_t)q * SD], geo);
            double acc[NTAB][VDIM];
            for (int tt = 0; tt < NTAB; ++tt)
                for (int v = 0; v < VDIM; ++v) acc[tt][v] = 0.0;
            fxk::eval_walk<SD, ORDER, VDIM>(c.n, t.phi0, t.coef.data(), w.data(), t.nexp, geo, acc);
            if constexpr (VDIM == SD && SD >= 2) {
                if (c.mapping != 0) {
                    double M[SD][SD];
                    fxk::eval_piola_matrix<SD>(c.verts.data(), G, c.mapping, M);
                    fxk::eval_apply_piola<SD, NTAB>(acc, M);
                }
            }
            for (int tt = 0; tt < NTAB; ++tt)
                for (int v = 0; v < VDIM; ++v) res[(((size_t)tt * c.nrhs + j) * VDIM + v) * c.npts + q] = acc[tt][v];
        }
    }
}

template <int SD, int VDIM> void run_order(int order, const Case& c, const fx::EvalTables& t, const std::vector<double>& Ap, std::vector<double>& res) {
    if (order == 0) run<SD, 0, VDIM>(c, t, Ap, res);
    else if (order == 1) run<SD, 1, VDIM>(c, t, Ap, res);
    else run<SD, 2, VDIM>(c, t, Ap, res);
}

bool dispatch(int order, const Case& c, const fx::EvalTables& t, const std::vector<double>& Ap, std::vector<double>& res) {
    if (c.sd == 1 && c.vdim == 1) run_order<1, 1>(order, c, t, Ap, res);
    else if (c.sd == 2 && c.vdim == 1) run_order<2, 1>(order, c, t, Ap, res);
    else if (c.sd == 2 && c.vdim == 2) run_order<2, 2>(order, c, t, Ap, res);
    else if (c.sd == 3 && c.vdim == 1) run_order<3, 1>(order, c, t, Ap, res);
    else if (c.sd == 3 && c.vdim == 3) run_order<3, 3>(order, c, t, Ap, res);
    else return false;
    return true;
}

double rel_error(const double* got, const double* ref, size_t count) {
    double err = 0.0, big = 1.0;
    for (size_t i = 0; i < count; ++i) {
        err = std::max(err, std::fabs(got[i] - ref[i]));
        big = std::max(big, std::fabs(ref[i]));
    }
    return err / big;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int ncases = 0;
    if (fscanf(f, "%d", &ncases) != 1 || ncases < 0) {
        fclose(f);
        return 2;
    }
    std::set<std::vector<int>> reached;
    int status = 0;
    for (int k = 0; k < ncases; ++k) {
        Case c;
        std::vector<double> scale;
        if (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &c.sd, &c.n, &c.variant, &c.order, &c.vdim, &c.mapping, &c.ndof, &c.nrhs, &c.npts,
                   &c.has_verts) != 10 ||
            c.sd < 1 || c.sd > 3 || c.n < 1 || c.n > fxk::EVAL_MAXK || c.variant < 0 || c.variant > 1 || c.order < 0 ||
            c.order > fxk::EVAL_MAXORDER || (c.vdim != 1 && c.vdim != c.sd) || c.mapping < 0 || c.mapping > 2 || c.ndof < 1 || c.nrhs < 1 ||
            c.npts < 0 || (c.mapping != 0 && !c.has_verts)) {
            fprintf(stderr, "case %d: malformed header\n", k);
            fclose(f);
            return 2;
        }
        const int nexp = fxk::eval_binom(c.n + c.sd, c.sd), ntab = fxk::eval_binom(c.sd + c.order, c.sd);
        bool ok = read_doubles(f, 1, scale) && read_doubles(f, (size_t)(c.sd + 1) * c.sd, c.cell);
        if (ok && c.has_verts) ok = read_doubles(f, (size_t)(c.sd + 1) * c.sd, c.verts);
        ok = ok && read_doubles(f, (size_t)c.ndof * c.vdim * nexp, c.coeffs) && read_doubles(f, (size_t)c.nrhs * c.ndof, c.dofs) &&
             read_doubles(f, (size_t)c.npts * c.sd, c.pts) && read_doubles(f, (size_t)ntab * c.nrhs * c.vdim * c.npts, c.ref);
        if (!ok) {
            fprintf(stderr, "case %d: malformed arrays\n", k);
            fclose(f);
            return 2;
        }
        c.scale = scale[0];
        const fx::EvalTables t = fx::eval_tables(c.sd, c.n, c.variant, c.scale);
        const std::vector<double> Ap = fx::eval_fold(c.sd, c.n, c.variant, c.ndof, c.vdim, c.coeffs.data(), t.member);
        const size_t per = (size_t)c.nrhs * c.vdim * c.npts;  // one table
        for (int order = 0; order <= c.order; ++order) {
            std::vector<double> res;
            if (!dispatch(order, c, t, Ap, res)) return 2;
            reached.insert({c.sd, order, c.vdim});
            const double e0 = rel_error(res.data(), c.ref.data(), per);
            const double e1 = order > 0 ? rel_error(res.data() + per, c.ref.data() + per, res.size() - per) : 0.0;
            const bool good = e0 <= 1e-12 && e1 <= 1e-10;
            printf("case %d eval_walk<%d,%d,%d> degree %d variant %d mapping %d verts %d: values %.2e derivatives %.2e%s\n", k, c.sd, order,
                   c.vdim, c.n, c.variant, c.mapping, c.has_verts, e0, e1, good ? "" : "  FAIL");
            if (!good) status = 1;
        }
    }
    fclose(f);
    int missing = 0;
    for (int sd = 1; sd <= 3; ++sd)
        for (int order = 0; order <= fxk::EVAL_MAXORDER; ++order)
            for (int vdim : {1, sd})
                if (!reached.count({sd, order, vdim})) {
                    printf("instance <%d,%d,%d> not reached\n", sd, order, vdim);
                    ++missing;
                }
    printf("%d cases, %zu instances, %d missing\n", ncases, reached.size(), missing);
    if (missing && status == 0) status = 2;
    return status;
}
