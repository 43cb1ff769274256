// Host-only check of the P1 tile records (fem-elastoplasticity_amd/csrc/fep_host.h, P1Plan::rec): what the tile kernels
// fetch at entry must decode to exactly the plan's descriptor, element runs and node runs.
//   tile_record_host MESHFILE
// MESHFILE as for host_san.cpp: int32 n_p (= 3), n_e, n_n, then the elements (3 x n_e, C order).  Builds the default plan
// and the variants that change what a record holds (one / four segments, list form, two-kernel plan), decodes every
// record with the kernels' own decoder (fep_layout.h: unpack_tile_head, run_entry) and compares with the plan's own tables.
// Prints one line per plan; exit code 0 = all records decode, 1 = a mismatch, 2 = unreadable mesh file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fem-elastoplasticity_amd/csrc/fep_host.h"

using namespace fep_host;

// 0, or the number of the first failed check
static int check_records(const P1Plan& P) {
    if (kRecInts * sizeof(int32_t) != 256 || (kRecInts * sizeof(int32_t)) % 64 != 0) return 1;            // stride, alignment
    if ((kRecRng * sizeof(int32_t)) % 64 != 0 || (kRecNrng * sizeof(int32_t)) % 64 != 0) return 1;        // each run table on a line of its own
    if ((int64_t)P.rec.size() != P.n_wg * kRecInts) return 2;
    for (int64_t g = 0; g < P.n_wg; ++g) {
        const int32_t* r = P.rec.data() + g * kRecInts;
        const int32_t* d = P.tdesc.data() + g * kDescInts;
        for (int i = 0; i < kDescInts; ++i)
            if (r[i] != d[i]) return 3;
        for (int i = kDescInts; i < kRecRng; ++i)
            if (r[i] != 0) return 4;                                                                     // padding
        // the descriptor's fields as the kernels unpack them
        const TileHead h = tile_head(r);
        const int nseg = h.nseg, n_el = h.n_el, n_nd = h.n_nd, nn = h.nn, n_own = h.n_own;
        int nb = 0, nnodes = 0;
        for (int s = 0; s < kSegMax; ++s) {
            if (s >= nseg && (r[4 + 4 * s] | r[5 + 4 * s] | r[6 + 4 * s] | r[7 + 4 * s]) != 0) return 5;  // unused segments are empty
            nb += r[5 + 4 * s]; nnodes += r[7 + 4 * s];
        }
        if (nb != r[1] || nnodes != nn || nseg < 1 || nseg > kSegMax) return 6;
        // the ends of the segments' output images fit the fields the kernels pack them into
        if (2 * nb > 1023 || nnodes > 255) return 7;
        const int32_t* er = r + kRecRng;
        const int32_t* nr = r + kRecNrng;
        if (P.lds && P.rng) {
            if (n_el < 1 || n_el > P.L || er[15] != n_el) return 8;
            for (int i = 0; i < P.L; ++i)
                if (run_entry(er, i) != P.elist_pad[(size_t)(g * P.L + i)]) return 9;
            for (int k = 0; k < 16; ++k)
                if (er[k] != P.rng_tab[(size_t)g * 16 + k]) return 10;
        } else {
            for (int k = 0; k < 16; ++k)
                if (er[k] != 0) return 11;                                                               // list form: no live run
        }
        if (P.fused && P.fused_rng) {
            if (n_nd < 1 || n_nd > P.NL || nr[15] != n_nd || n_own > n_el) return 12;
            for (int i = 0; i < P.NL; ++i)
                if (run_entry(nr, i) != P.nlist_pad[(size_t)(g * P.NL + i)]) return 13;
            for (int k = 0; k < 16; ++k)
                if (nr[k] != P.nrng_tab[(size_t)g * 16 + k]) return 14;
        } else {
            for (int k = 0; k < 16; ++k)
                if (nr[k] != 0) return 15;
        }
        // a run table that is not in use never decodes as a live run: cumulative count 0 at every slot
        if (!(P.lds && P.rng) && er[15] != 0) return 16;
        if (!(P.fused && P.fused_rng) && nr[15] != 0) return 16;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] != 3) return 2;
    const int64_t n_e = hdr[1], n_n = hdr[2];
    std::vector<int32_t> elem(3 * (size_t)n_e);
    if (std::fread(elem.data(), sizeof(int32_t), elem.size(), f) != elem.size()) return 2;
    std::fclose(f);
    Symbolic S;
    if (build_symbolic(3, n_e, n_n, elem.data(), S) != FEP_OK) return 1;
    struct Case { const char* name; bool rng, pk, fused; int segs; };
    const Case cases[] = {{"default", true, true, true, 2}, {"one segment", true, true, true, 1}, {"lists", false, true, true, 2},
                          {"unpacked", true, false, true, 2}, {"two kernels", true, true, false, 2}, {"four segments", true, true, true, 4}};
    int rc = 0;
    for (const Case& cs : cases) {
        P1Options opt;
        opt.allow_rng = cs.rng; opt.allow_pk = cs.pk; opt.allow_fused = cs.fused; opt.max_segs = cs.segs;
        P1Plan P;
        const int r = build_p1_plan(S, n_e, n_n, elem.data(), opt, P);
        const int bad = r == FEP_OK ? validate_p1_plan(P, S, n_e, n_n, elem.data()) : -1;
        const int rec = r == FEP_OK ? check_records(P) : -1;
        std::printf("records [%s]: rc %d check %d record %d tiles %lld segs %d lds %d rng %d pk %d fused %d/%d bytes %zu\n", cs.name, r, bad,
                    rec, (long long)P.n_wg, P.n_segs, (int)P.lds, (int)P.rng, (int)P.pk, (int)P.fused, (int)P.fused_rng,
                    P.rec.size() * sizeof(int32_t));
        if (r != FEP_OK || bad || rec) rc = 1;
    }
    std::printf("result %s\n", rc ? "FAILED" : "ok");
    return rc;
}
