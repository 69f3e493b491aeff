// Host program around vicasplat_amd/csrc/routes.h for tests/test_routes_cpu.py.  One query per line of stdin, one answer per line:
//   g <f16|bf16|f32x|split> M N K epi resid a_packed out_packed deterministic   -> the plan in the format of tests/gemm_f64.py plan()
//   c dtype Nimg H W Cin Cout stride a_packed  (H, W of the output, Cin in channels) -> "<kind> kpt=.. grid=.." / "wave4 mi=.. grid=.."
#include <cstdio>
#include <cstring>
#include <string>

#include "../vicasplat_amd/csrc/routes.h"

using namespace vs::route;

static std::string step_name(const GemmStep &s, bool tail) {
    char b[64];
    const int rows = s.m_hi - s.m_lo;
    switch (s.leaf) {
        case Leaf::SmallM: snprintf(b, sizeof b, "smallm<NW%d,MF%d>", s.nw, s.mf); break;
        case Leaf::Skinny: snprintf(b, sizeof b, "skinny(ks=%d)", s.ksplit); break;
        default: {
            const char *n = s.leaf == Leaf::G256 ? "g256" : s.leaf == Leaf::Mi2 ? "mi2" : s.leaf == Leaf::Mi4 ? "mi4" : "mi8";
            if (tail) snprintf(b, sizeof b, "%s(ks=%d)", n, s.ksplit);
            else snprintf(b, sizeof b, "%s(rows=%d)", n, rows);
        }
    }
    return b;
}

int main() {
    char line[256], cls[16];
    while (fgets(line, sizeof line, stdin)) {
        int a[9];
        if (sscanf(line, "g %15s %d %d %d %d %d %d %d %d", cls, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) == 9) {
            const int c = !strcmp(cls, "f16") ? 0 : !strcmp(cls, "bf16") ? 1 : !strcmp(cls, "f32x") ? kF32 : !strcmp(cls, "split") ? kSplit : -1;
            if (c < 0) return 2;
            const GemmPlan p = gemm_plan(c, a[0], a[1], c >= kF32 ? 2 * a[2] : a[2], a[3], a[4] != 0, a[5] != 0, a[6] != 0, a[7] != 0);
            std::string out = step_name(p.step[0], false);
            if (p.step[0].m_lo != 0 || p.step[p.n - 1].m_hi != a[0]) return 3;      // the steps cover [0, M) once
            if (p.n == 2) {
                if (p.step[0].m_hi != p.step[1].m_lo) return 3;
                out += "+tail:" + step_name(p.step[1], true);
            }
            puts(out.c_str());
        } else if (sscanf(line, "c %d %d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) == 8) {
            const ConvRoute r = conv3x3_route(a[0], (long long)a[1] * a[2] * a[3], a[2], a[3], a[0] >= 3 ? 2 * a[4] : a[4], a[5], a[6], a[7] != 0);
            static const char *kinds[] = {"halo256", "tile256", "tile256x128", "wave4", "packed_not_taken"};
            if (r.kind == ConvKind::Wave4) printf("wave4 mi=%d grid=%lld\n", r.mi, r.grid);
            else if (r.kind == ConvKind::PackedNotTaken) puts("packed_not_taken");
            else printf("%s kpt=%d grid=%lld\n", kinds[(int)r.kind], r.kpt, r.grid);
        } else {
            return 1;
        }
    }
    return 0;
}
