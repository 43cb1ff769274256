// Host-only digest of every table the planner (fem-elastoplasticity_amd/csrc/fep_host.h) builds for a mesh.
//   plan_digest_host MESHFILE
// MESHFILE as for host_san.cpp: int32 n_p, n_e, n_n, then the elements (n_p x n_e, C order), optionally 2 x n_n doubles of
// coordinates.  Prints one line per (plan variant, table): the table's length and the 64-bit FNV-1a digest of its bytes;
// every vector of P1Plan for the six variants of tile_record_host.cpp (P1 meshes), every vector of PatchPlan for the
// (n_p, eb, PatchOptions) rows of host_san.cpp.  Two builds of the planner that print the same lines built the same
// tables; so do two runs with different FEP_HOST_THREADS (tests/test_plan_digest_host.py).  No digest is pinned anywhere:
// the formats may change.  Uses member names only, so it compiles against any version of fep_host.h that has them.
// Exit code 0, or 1 = a plan could not be built, 2 = unreadable mesh file.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fem-elastoplasticity_amd/csrc/fep_host.h"

using namespace fep_host;

template <class T> static void line(const char* plan, const char* table, const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    std::printf("%s %s %zu %016llx\n", plan, table, v.size(), (unsigned long long)h);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int n_p = hdr[0];
    const int64_t n_e = hdr[1], n_n = hdr[2];
    std::vector<int32_t> elem((size_t)n_p * n_e);
    if (std::fread(elem.data(), sizeof(int32_t), elem.size(), f) != elem.size()) return 2;
    std::vector<double> xy(2 * (size_t)n_n);
    if (std::fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) {      // no coordinates: host_san.cpp's lattice stands in
        const int64_t side = (int64_t)std::ceil(std::sqrt((double)n_n));
        for (int64_t n = 0; n < n_n; ++n) { xy[n] = (double)(n % side); xy[n_n + n] = (double)(n / side); }
    }
    std::fclose(f);
    Symbolic S;
    if (build_symbolic(n_p, n_e, n_n, elem.data(), S) != FEP_OK) return 1;
    line("symbolic", "iptr", S.iptr); line("symbolic", "ilist", S.ilist); line("symbolic", "nptr", S.nptr);
    line("symbolic", "ncol", S.ncol); line("symbolic", "segptr", S.segptr); line("symbolic", "perm", S.perm);
    line("symbolic", "meta", S.meta);
    int rc = 0;
    char name[96];
    if (n_p == 3) {
        struct Case { const char* name; bool rng, pk, fused; int segs; };
        const Case cases[] = {{"default", true, true, true, 2}, {"one-segment", true, true, true, 1}, {"lists", false, true, true, 2},
                              {"unpacked", true, false, true, 2}, {"two-kernels", true, true, false, 2}, {"four-segments", true, true, true, 4}};
        for (const Case& cs : cases) {
            P1Options opt;
            opt.allow_rng = cs.rng; opt.allow_pk = cs.pk; opt.allow_fused = cs.fused; opt.max_segs = cs.segs;
            P1Plan P;
            const int r = build_p1_plan(S, n_e, n_n, elem.data(), opt, P);
            std::snprintf(name, sizeof name, "p1[%s]", cs.name);
            std::printf("%s scalars rc %d tile %d segs %d tiles %lld staged %lld nodes %lld lds %d rng %d pk %d fused %d/%d L %d C %d NL %d\n",
                        name, r, P.tile, P.n_segs, (long long)P.n_wg, (long long)P.staged_total, (long long)P.staged_nodes_total,
                        (int)P.lds, (int)P.rng, (int)P.pk, (int)P.fused, (int)P.fused_rng, P.L, P.C, P.NL);
            if (r != FEP_OK) { rc = 1; continue; }
            line(name, "tdesc", P.tdesc); line(name, "rec", P.rec); line(name, "perm2", P.perm2);
            line(name, "elist_pad", P.elist_pad); line(name, "rng_tab", P.rng_tab); line(name, "nlist_pad", P.nlist_pad);
            line(name, "nrng_tab", P.nrng_tab); line(name, "codes_pad", P.codes_pad); line(name, "pkv", P.pkv);
            line(name, "elnodes", P.elnodes);
        }
    }
    const int ebs_np[][4] = {{3, 64, 7, 1}, {6, 56, 28, 5}, {4, 64, 9, 2}, {8, 28, 24, 3}, {15, 16, 4, 1}};     // host_san.cpp's rows
    for (const auto& row : ebs_np) {
        if (row[0] != n_p) continue;
        for (int k = 1; k < 4; ++k)
            for (int variant = 0; variant < 4; ++variant) {
                PatchOptions opt;
                opt.order = variant == 3 ? 2 : variant;
                opt.runs = variant == 3 ? 4 : 2;
                opt.align = variant == 2 ? 16 : 1;
                PatchPlan P;
                const int r = build_patch_plan(S, n_p, n_e, n_n, elem.data(), xy.data(), row[k], opt, P);
                std::snprintf(name, sizeof name, "patch[eb%d,order%d,runs%d,align%d]", row[k], opt.order, opt.runs, opt.align);
                std::printf("%s scalars rc %d ok %d eb %d max_items %d max_fitems %d patches %lld open %lld part %lld fopen %lld fpart %lld\n",
                            name, r, (int)P.ok, P.eb, P.max_items, P.max_fitems, (long long)P.n_patch, (long long)P.n_open,
                            (long long)P.n_part, (long long)P.n_fopen, (long long)P.n_fpart);
                if (r != FEP_OK) { rc = 1; continue; }
                line(name, "pdesc", P.pdesc); line(name, "plist", P.plist); line(name, "pel", P.pel); line(name, "pnodes", P.pnodes);
                line(name, "items", P.items); line(name, "fitems", P.fitems); line(name, "codes", P.codes); line(name, "fcodes", P.fcodes);
                line(name, "fix", P.fix); line(name, "ffix", P.ffix); line(name, "fixT", P.fixT);
            }
    }
    return rc;
}
