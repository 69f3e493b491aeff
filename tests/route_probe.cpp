// Host program around vicasplat_amd/csrc/routes.h for tests/test_routes_cpu.py.  One query per line of stdin, one answer per line:
//   g <f16|bf16|f32x|split> M N K epi resid a_packed out_packed deterministic   -> the plan in the format of tests/gemm_f64.py plan()
//   c dtype Nimg H W Cin Cout stride a_packed  (H, W of the output, Cin in channels) -> "<kind> kpt=.. grid=.." / "wave4 mi=.. grid=.."
//   a <f16|bf16|f32x|split|sp> nbatch H Lq Lk has_seg has_len  (Lk as the ABI receives it) -> "<kind> grid=XxYxZ" (res: + " block=512") / "sp grid=.."
//   b <16|split> Lq Lk has_seg max_keys                         -> "keys=.. dq=.. dkv=.."  (x-extents of the backward's two grids)
//   x n  -> "ok" if xcd_remap(., n) is a permutation of [0, n) and the ids that share an XCD (equal id % 8) map to one contiguous range, else
//           "bad <first offending id>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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
        } else if (sscanf(line, "a %15s %d %d %d %d %d %d", cls, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
            const int dt = !strcmp(cls, "f16") ? 1 : !strcmp(cls, "bf16") ? 2 : !strcmp(cls, "f32x") ? 3 : !strcmp(cls, "split") || !strcmp(cls, "sp") ? 4 : -1;
            if (dt < 0) return 2;
            const AttnRoute r = attention_route(dt, !strcmp(cls, "sp"), a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0);
            static const char *kinds[] = {"res", "tile64", "tile128", "f32", "split64", "split128", "sp"};
            if (r.block != (r.kind == AttnKind::Res ? 512 : 256)) return 3;
            if (r.kind == AttnKind::Packed96) printf("sp grid=%lld\n", r.gx);
            else printf("%s grid=%lldx%dx%d%s\n", kinds[(int)r.kind], r.gx, r.gy, r.gz, r.kind == AttnKind::Res ? " block=512" : "");
        } else if (sscanf(line, "b %15s %d %d %d %d", cls, &a[0], &a[1], &a[2], &a[3]) == 5) {
            const AttnBwdRoute r = attention_bwd_route(!strcmp(cls, "split"), a[0], a[1], a[2] != 0, a[3]);
            printf("keys=%d dq=%d dkv=%d\n", r.keys, r.gq, r.gk);
        } else if (sscanf(line, "x %d", &a[0]) == 1) {
            const int n = a[0];
            if (n < 1) return 2;
            std::vector<char> seen(n, 0);
            int bad = -1;
            for (int xcd = 0; xcd < 8 && bad < 0; ++xcd) {
                int lo = n, hi = -1, cnt = 0;      // the logical ids of the workgroups this XCD receives
                for (int id = xcd; id < n; id += 8, ++cnt) {
                    const int l = xcd_remap(id, n);
                    if (l < 0 || l >= n || seen[l]) { bad = id; break; }
                    seen[l] = 1;
                    lo = l < lo ? l : lo;
                    hi = l > hi ? l : hi;
                }
                // distinct ids in a range as long as their count are contiguous; otherwise the first id that lands past [lo, lo + cnt)
                if (bad < 0 && cnt > 0 && hi - lo + 1 != cnt)
                    for (int id = xcd; bad < 0; id += 8)
                        if (xcd_remap(id, n) >= lo + cnt) bad = id;
            }
            if (bad < 0) puts("ok");
            else printf("bad %d\n", bad);
        } else {
            return 1;
        }
    }
    return 0;
}
