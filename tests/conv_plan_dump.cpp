// Prints the plan of a sweep of conv launches, one line per case: what nope::conv_plan decides (every scalar of the kernels' parameters,
// which pointers are set, grid, kernel, tile, precision, reduce kernel, error code) and what the eight query functions answer.
// Host code only: built against tests/hipemu/include and linked to the interpreter library (tests/hipemu/build_emu.py); launches nothing.
//
//   conv_plan_dump table [K0 K1]    the thinned sweep that tests/conv_plan_table.txt records (tests/test_conv_plan.py)
//   conv_plan_dump full E D         one shard of the full sweep: environment setting E (0..39), compute type D (0..5); the sweep, then the GroupNorm-tail launches
//
// A deliberate change of the dispatch policy changes the table: regenerate it with
//   python tests/test_conv_plan.py --regenerate
// and review the diff line by line -- each changed line is a launch that now runs differently.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_plan.h"

using namespace nope;

struct EnvSetting { const char* text; };      // "NAME=VALUE NAME=VALUE", "" = every switch unset
static const EnvSetting kEnvs[] = {
    {""},
    {"NOPE_CONV_PP=0"}, {"NOPE_CONV_PP=7"}, {"NOPE_CONV_PP=11"}, {"NOPE_CONV_PP=19"},
    {"NOPE_CONV_SMALL=0"}, {"NOPE_CONV_SMALL=2"},
    {"NOPE_SMALL_TILE=0"}, {"NOPE_SMALL_TILE=1"}, {"NOPE_SMALL_TILE=2"}, {"NOPE_SMALL_TILE=3"},
    {"NOPE_CONV_STREAM=1 NOPE_STREAM_GRID=8"}, {"NOPE_CONV_STREAM=3 NOPE_STREAM_GRID=8"},
    {"NOPE_CONV_VARIANT=4"}, {"NOPE_HALO_SPLIT=0"}, {"NOPE_HALO_PERSIST=8"}, {"NOPE_XCD_MAP=1"}, {"NOPE_XCD_GN=2"}, {"NOPE_XCD_ANY=0"},
    {"NOPE_CONV_PERSIST=0"}, {"NOPE_EPILOGUE_LEAN=0"}, {"NOPE_STATS16=0"}, {"NOPE_UP2P_HALO=0"}, {"NOPE_UP2P_HALO=2"}, {"NOPE_X2_PP=0"},
    {"NOPE_X2_SMALL=1"}, {"NOPE_GEGLU_FUSED=2"},
    // 27..: one setting per switch the settings above leave alone
    {"NOPE_SMALL_MAX_TILES=64"}, {"NOPE_SMALL_1X1_MAXK=3"}, {"NOPE_SMALL_DEEP_MAX=512"}, {"NOPE_SMALL_KG2_MAX=0"},
    {"NOPE_HALO_SPLIT_MIN_CHUNKS=4"}, {"NOPE_HALO_SPLIT_MAX_TILES=64"}, {"NOPE_HALO_MIN_TILES=256"},
    {"NOPE_CONV_STREAM=1 NOPE_STREAM_GRID=8 NOPE_STREAM_MIN_ITERS=128"}, {"NOPE_GEGLU_FUSED_F32=0"}, {"NOPE_NCHW_STAGED=0"}, {"NOPE_PERSIST_GRID=256"},
    {"NOPE_PP_VARIANT=1"}, {"NOPE_GEGLU_FUSED=0"},
};
constexpr int kNumEnvs = (int)(sizeof(kEnvs) / sizeof(kEnvs[0]));
extern char** environ;

static void set_env(int e) {
    char buf[128];
    for (bool again = true; again;) {      // every NOPE_* variable, whatever switches the library has by now (unsetenv moves `environ`: start over)
        again = false;
        for (char** v = environ; *v; ++v)
            if (!strncmp(*v, "NOPE_", 5) && strchr(*v, '=')) {
                const size_t n = (size_t)(strchr(*v, '=') - *v);
                if (n >= sizeof(buf)) continue;
                memcpy(buf, *v, n); buf[n] = 0;
                unsetenv(buf);
                again = true;
                break;
            }
    }
    strncpy(buf, kEnvs[e].text, sizeof(buf) - 1); buf[sizeof(buf) - 1] = 0;
    for (char* tok = strtok(buf, " "); tok; tok = strtok(nullptr, " ")) {
        char* eq = strchr(tok, '=');
        *eq = 0;
        setenv(tok, eq + 1, 1);
    }
    nope_tuning_reload();
}

// compute types: the last two are NOPE_BF16X3 with the second weight pack, and NOPE_F16X2 as an element type
struct DtCase { int dt; bool w_x2; const char* name; };
static const DtCase kDts[] = {{NOPE_F32, false, "f32"}, {NOPE_BF16, false, "bf16"}, {NOPE_F16, false, "f16"}, {NOPE_BF16X3, false, "bf16x3"},
                              {NOPE_BF16X3, true, "bf16x3+x2"}, {NOPE_F16X2, false, "f16x2"}};
struct ModeCase { int mode, ntaps; };
static const ModeCase kModes[] = {{NOPE_CONV_PLAIN, 1}, {NOPE_CONV_PLAIN, 9}, {NOPE_CONV_UP2, 9}, {NOPE_CONV_DOWN2, 4}, {NOPE_CONV_UP2P, 4},
                                  {NOPE_CONV_STRIDE2, 1}, {NOPE_CONV_STRIDE2, 9}, {NOPE_CONV_STRIDE2, 16}, {NOPE_CONV_STRIDE2_PAD01, 9}};
static const int kCin[][2] = {{8, 0}, {64, 0}, {100, 0}, {192, 0}, {320, 0}, {384, 384}, {768, 0}, {1280, 0}, {1536, 1536}};
static const int kCout[] = {8, 100, 192, 320, 384, 960, 1280, 1536};
static const int kSide[] = {4, 8, 16, 30, 32, 34};      // both sides of HALO_MAX_W, of the Ws <= 30 bound of the UP2P tap-resident form, of POSMAJOR_MAX_HW
static const int kNhyp[] = {1, 26, 64, 128, 256, 341, 512};
enum { F_RESID = 1, F_NCHW = 2, F_ACT = 4, F_STATS = 8, F_PRENORM = 16, F_GEGLU = 32 };

alignas(16) static int g_dummy[4];      // every pointer of a case points here; nothing dereferences them

static void print_plan(const ConvLaunch& L) {
    const ConvParams& p = L.p;
    printf("dt %d C %d,%d rep %d,%d src %dx%d out %dx%d grid %dx%d mode %d taps %d s2 %d Cout %d M %d nchw %d,%d,%d act %d tiles %dx%d xcd %d/%d wide %d geglu %d variant %d "
           "div %u.%u,%u.%u,%u.%u,%u.%u,%u.%u nhyp %d persist %d,%u,%u,%d posmajor %d splits %d wph %u stat_rows %d bytes %u,%u,%u t_zero %d lean %d",
           L.dt, p.C1, p.C2, p.rep1, p.rep2, p.Hs, p.Ws, p.Ho, p.Wo, p.Hm, p.Wm, p.mode, p.ntaps, p.s2_off, p.Cout, p.M, p.out_nchw, p.out_dt, p.nchw_staged, p.act,
           p.tiles_m, p.tiles_n, p.xcd_map, p.xcd_gn, p.wide_out, p.geglu, p.variant,
           p.d_hw.M, p.d_hw.sh, p.d_w.M, p.d_w.sh, p.d_rep1.M, p.d_rep1.sh, p.d_rep2.M, p.d_rep2.sh, p.d_n.M, p.d_n.sh, p.nhyp,
           p.persist_iters, p.persist_d1, p.persist_d2, p.persist_dm, p.posmajor, p.splits, p.w_phase_bytes, p.stat_rows, p.bytes1, p.bytes2, p.bytesw, p.x2_t_zero, p.lean);
    if (p.posmajor) { printf(" order "); for (int i = 0; i < p.Hs * p.Ws; ++i) printf("%02x", p.pos_order[i]); }
    // pointers, set or not: src1 src2 w bias resid out timeline split_out colstats pn_ms pn_c0 pn_c1 x2_scale x2_amax out_amax; where the two-pass scale sits behind w
    const void* const ptrs[] = {p.src1, p.src2, p.w, p.bias, p.resid, p.out, p.timeline, p.split_out, p.colstats, p.pn_ms, p.pn_c0, p.pn_c1, p.x2_scale, p.x2_amax, p.out_amax};
    printf(" ptr ");
    for (const void* q : ptrs) putchar(q ? '1' : '0');
    printf(" scale_at %lld", p.x2_scale ? (long long)((const unsigned char*)p.x2_scale - p.w) : -1LL);
    printf(" launch %u,%u,%u kind %d small %d bm %d x2 %d reduce %d", L.grid.x, L.grid.y, L.grid.z, L.kind, L.small, L.bm, L.x2 ? 1 : 0, L.reduce);
    // GroupNorm tail (ConvArgs::gn_*): groups, the divider by channels per group, wave-tile columns; gn_ms gn_gamma gn_beta tail_stats, set or not
    if (p.gn_ms) printf(" gn_G %d d_cpg %u.%u tail_cols %d tail %d%d%d%d", p.gn_G, p.d_cpg.M, p.d_cpg.sh, p.tail_cols, p.gn_ms ? 1 : 0, p.gn_gamma ? 1 : 0, p.gn_beta ? 1 : 0, p.tail_stats ? 1 : 0);
}

// One case: the arguments as a runtime would fill them (statistics and split-K scratch asked for first), the plan, the queries.
// accepted_only: print nothing for a launch conv_plan refuses.  Returns whether a line was printed.
static bool plan_line(int e, const DtCase& d, const ModeCase& mc, const int* cin, int cout, int side, int nhyp, int rep1, int flags, int ws, bool accepted_only = false,
                      int gn_G = 0, bool tail_stats = false) {      // gn_G > 0: with a GroupNorm tail on the residual
    ConvArgs a;
    a.src1 = g_dummy; a.C1 = cin[0]; a.rep1 = rep1;
    if (cin[1]) { a.src2 = g_dummy; a.C2 = cin[1]; }
    a.Hs = a.Ws = side;
    const bool up = mc.mode == NOPE_CONV_UP2 || mc.mode == NOPE_CONV_UP2P, half = mc.mode == NOPE_CONV_DOWN2 || mc.mode >= NOPE_CONV_STRIDE2;
    a.Ho = a.Wo = up ? 2 * side : half ? side / 2 : side;
    a.mode = mc.mode; a.ntaps = mc.ntaps; a.w = g_dummy; a.bias = (const float*)g_dummy; a.out = g_dummy; a.Cout = cout; a.nhyp = nhyp;
    if (d.w_x2) { a.w_x2 = g_dummy; a.x2_t_zero = 1; }
    a.x2_amax = (unsigned*)g_dummy; a.out_amax = (unsigned*)g_dummy;
    if (flags & F_RESID) a.resid = g_dummy;
    if (flags & F_NCHW) a.out_nchw = 1;
    if (flags & F_ACT) a.act = 1;
    if (flags & F_PRENORM) { a.pn_ms = a.pn_c0 = a.pn_c1 = (const float*)g_dummy; }
    if (flags & F_GEGLU) a.geglu = 1;
    if (gn_G) { a.gn_ms = a.gn_gamma = a.gn_beta = (const float*)g_dummy; a.gn_G = gn_G; if (tail_stats) a.tail_stats = (float*)g_dummy; }
    const int stat_rows = conv_stat_rows(d.dt, a);
    if (flags & F_STATS) {
        if (stat_rows == 0) return false;      // (no statistics from this shape: the caller does not ask)
        a.colstats = (float*)g_dummy; a.stat_rows = stat_rows;
    }
    const int S = conv_splitk_factor(d.dt, a);
    if (ws) {
        if (ws == 2 && S <= 1) return false;      // (one byte short of nothing)
        a.splitk_ws = g_dummy;
        a.splitk_bytes = (size_t)S * nhyp * a.Ho * a.Wo * cout * 4 - (ws == 2 ? 1 : 0);
    }
    const ConvLaunch L = conv_plan(d.dt, a);
    const int err = L.err;
    if (err != NOPE_OK && accepted_only) return false;
    printf("env %d %s mode %d taps %d Cin %d+%d Cout %d side %d nhyp %d rep1 %d flags %d ws %d", e, d.name, mc.mode, mc.ntaps, cin[0], cin[1], cout, side, nhyp, rep1, flags, ws);
    if (gn_G) printf(" gn %d,%d", gn_G, tail_stats ? 1 : 0);
    printf(" | ");
    if (err == NOPE_OK) print_plan(L);
    printf(" | err %d stat_rows %d splitk %d", err, stat_rows, S);
    if (err == NOPE_OK)      // (of a launch that is refused there is no plan to ask about)
        printf(" posmajor %d kind %d x2 %d amax %d flops %.17g geglu_ok %d", conv_is_posmajor(d.dt, a) ? 1 : 0, conv_kernel_kind(d.dt, a), conv_takes_x2(d.dt, a) ? 1 : 0,
               conv_records_out_amax(d.dt, a) ? 1 : 0, conv_executed_flops(d.dt, a), conv_geglu_fusable(d.dt, a) ? 1 : 0);
    putchar('\n');
    return true;
}

// flag combinations launch_conv does not refuse outright
static bool flags_ok(const ModeCase& mc, int flags) {
    const bool one_by_one = mc.mode == NOPE_CONV_PLAIN && mc.ntaps == 1;
    if ((flags & F_GEGLU) && (!one_by_one || flags != F_GEGLU)) return false;
    if ((flags & F_PRENORM) && (!one_by_one || (flags & F_STATS))) return false;
    if ((flags & F_STATS) && (flags & (F_RESID | F_NCHW | F_ACT) || mc.mode == NOPE_CONV_UP2P)) return false;
    if ((flags & F_NCHW) && mc.mode == NOPE_CONV_UP2P) return false;
    return true;
}
static bool two_sources_ok(const ModeCase& mc) { return mc.mode == NOPE_CONV_PLAIN || mc.mode == NOPE_CONV_UP2 || mc.mode == NOPE_CONV_DOWN2; }

// `keep`: 0 = every case, else every keep-th case, or the next one after it that conv_plan accepts (the table)
static void sweep(int e, const DtCase& d, const int* nhyps, int n_nhyp, unsigned keep, unsigned& counter) {
    bool due = false;
    for (const ModeCase& mc : kModes)
        for (const auto& cin : kCin) {
            if (cin[1] && !two_sources_ok(mc)) continue;
            for (int cout : kCout)
                for (int side : kSide)
                    for (int k = 0; k < n_nhyp; ++k)
                        for (int r = 0; r < 2; ++r) {
                            const int nhyp = nhyps[k], rep1 = r ? nhyp : 1;
                            if (r && nhyp == 1) continue;
                            for (int flags = 0; flags < 64; ++flags) {
                                if (!flags_ok(mc, flags)) continue;
                                for (int ws = 0; ws < 3; ++ws) {
                                    if (keep && !(counter++ % keep)) due = true;
                                    if (keep && !due) continue;
                                    if (plan_line(e, d, mc, cin, cout, side, nhyp, rep1, flags, ws, keep != 0)) due = false;
                                }
                            }
                        }
        }
}

// The launches with a GroupNorm tail (ConvArgs::gn_*): 1x1 convs with a residual, refused ones included
static void sweep_tail(int e, const DtCase& d) {
    for (const auto& cin : kCin)
        for (int cout : kCout)
            for (int side : kSide)
                for (int nhyp : kNhyp)
                    for (int gn_G : {1, 32})
                        for (int ts = 0; ts < 2; ++ts) plan_line(e, d, kModes[0], cin, cout, side, nhyp, 1, F_RESID, 0, false, gn_G, ts != 0);
}

int main(int argc, char** argv) {
    unsigned counter = 0;
    if (argc == 4 && !strcmp(argv[1], "full")) {
        const int e = atoi(argv[2]), d = atoi(argv[3]);
        if (e < 0 || e >= kNumEnvs || d < 0 || d >= 6) return 2;
        set_env(e);
        sweep(e, kDts[d], kNhyp, 7, 0, counter);
        sweep_tail(e, kDts[d]);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "table")) {
        static const int table_envs[] = {0, 3, 6, 12, 17};      // unset; NOPE_CONV_PP=11; NOPE_CONV_SMALL=2; NOPE_CONV_STREAM=3 + NOPE_STREAM_GRID=8; NOPE_XCD_GN=2
        static const int table_nhyp[] = {26, 64, 256, 512};
        const unsigned keep0 = argc == 4 ? atoi(argv[2]) : 30011, keep1 = argc == 4 ? atoi(argv[3]) : 120011;      // every keep-th case: unset / switched settings
        printf("# The plan of a thinned sweep of conv launches (tests/conv_plan_dump.cpp table): case | plan | answers of the query functions.\n"
               "# A deliberate change of the dispatch policy changes these lines: python tests/test_conv_plan.py --regenerate, then review the diff.\n");
        for (int e : table_envs) {
            set_env(e);
            printf("# env %d: %s\n", e, kEnvs[e].text[0] ? kEnvs[e].text : "(every switch unset)");
            for (const DtCase& d : kDts) sweep(e, d, table_nhyp, 4, e == 0 ? keep0 : keep1, counter);
        }
        // one launch of every form the thinning above might miss (tests/test_conv_plan.py lists what a table must contain), and launches
        // conv_plan refuses (the sweep leaves out what is refused for its arguments alone)
        struct Witness { int env, dt; ModeCase mc; int cin, cout, side, nhyp, flags, ws, gn_G, tail_stats; };
        static const Witness witnesses[] = {
            {0, 0, {NOPE_CONV_PLAIN, 9}, 1, 320, 8, 512, 0, 0},              // position-major rows (f32 keeps the 128 x 192 kernel)
            {0, 1, {NOPE_CONV_PLAIN, 1}, 1, 8, 16, 512, 0, 0},               // tile walk: 128 x 192 kernel
            {0, 1, {NOPE_CONV_PLAIN, 9}, 3, 8, 16, 512, 0, 0},               //            tap-resident kernel
            {12, 1, {NOPE_CONV_PLAIN, 1}, 1, 8, 16, 256, 0, 0},              //            streaming kernel
            {0, 1, {NOPE_CONV_PLAIN, 9}, 5, 8, 4, 26, 0, 1},                 // K splits: tap-resident kernel, plain reduce
            {0, 1, {NOPE_CONV_PLAIN, 9}, 5, 8, 4, 26, F_STATS, 1},           //           ... reduce with statistics
            {0, 1, {NOPE_CONV_PLAIN, 9}, 5, 8, 4, 26, 0, 2},                 //           ... scratch one byte short: no split
            {3, 0, {NOPE_CONV_PLAIN, 1}, 4, 8, 4, 26, F_NCHW, 1},            //           128 x 192 kernel
            {3, 0, {NOPE_CONV_PLAIN, 1}, 4, 8, 4, 26, F_NCHW, 2},            //           ... scratch one byte short: no split
            {0, 4, {NOPE_CONV_PLAIN, 9}, 1, 8, 16, 256, 0, 0},               // two-pass tile: tap-resident
            {0, 4, {NOPE_CONV_PLAIN, 1}, 5, 8, 16, 256, 0, 0},               //                per tap
            {0, 4, {NOPE_CONV_UP2P, 4}, 3, 8, 8, 256, 0, 0},                 //                the phase convs of an up-sampling, tap-resident
            {0, 5, {NOPE_CONV_PLAIN, 9}, 1, 8, 16, 256, 0, 0},               //                NOPE_F16X2 as the element type: `w` holds the two-pass pack
            {0, 0, {NOPE_CONV_PLAIN, 1}, 1, 192, 4, 26, F_GEGLU, 0},         // GEGLU epilogue
            {0, 0, {NOPE_CONV_PLAIN, 1}, 0, 8, 8, 26, F_NCHW, 0},            // NCHW output through the LDS panels
            {0, 0, {NOPE_CONV_PLAIN, 1}, 0, 8, 4, 26, 0, 0},                 // workgroup -> tile map 0
            {0, 0, {NOPE_CONV_PLAIN, 1}, 1, 320, 4, 256, F_NCHW | F_PRENORM, 0},      // map 2
            {0, 0, {NOPE_CONV_PLAIN, 1}, 1, 8, 4, 64, 0, 0},                 // map 3
            {0, 0, {NOPE_CONV_PLAIN, 1}, 0, 960, 4, 64, 0, 0},               // map 4
            {0, 0, {NOPE_CONV_PLAIN, 4}, 3, 192, 8, 64, 0, 0},               // refused: a 2x2 conv without resampling
            {0, 3, {NOPE_CONV_PLAIN, 9}, 3, 192, 8, 64, F_PRENORM, 0},       //          PreNorm in front of a 3x3 conv
            {0, 3, {NOPE_CONV_PLAIN, 1}, 3, 192, 8, 64, F_STATS | F_ACT, 0}, //          statistics behind an activation
            {0, 1, {NOPE_CONV_STRIDE2, 9}, 5, 192, 8, 64, 0, 0},             //          a strided conv over two sources
            {0, 1, {NOPE_CONV_PLAIN, 1}, 2, 192, 8, 64, 0, 0},               //          100 channels: no whole 16-byte vectors of 16-bit elements
            {0, 0, {NOPE_CONV_PLAIN, 1}, 0, 8, 4, 26, F_GEGLU, 0},           //          GEGLU off the LDS-DMA kernel
            {0, 5, {NOPE_CONV_UP2, 9}, 3, 192, 8, 64, 0, 0},                 //          the two-pass weights alone on a kernel that cannot read them
            {0, 3, {NOPE_CONV_PLAIN, 1}, 5, 384, 16, 256, F_RESID, 0, 32, 1},       // GroupNorm tail: the per-tap ping-pong kernel's lean epilogue
            {0, 3, {NOPE_CONV_PLAIN, 9}, 3, 384, 16, 256, F_RESID, 0, 32, 1},       //   refused: a 3x3 conv that goes tap-resident
            {0, 3, {NOPE_CONV_PLAIN, 1}, 5, 384, 8, 26, F_RESID, 0, 32, 1},         //            a launch of the small-tile kernel
            {38, 3, {NOPE_CONV_PLAIN, 1}, 5, 384, 16, 256, F_RESID, 0, 32, 1},      //            the accepted launch under NOPE_PP_VARIANT=1 (the ablations have no tail)
        };
        printf("# one launch of every form, and refused launches\n");
        for (const Witness& w : witnesses) {
            set_env(w.env);
            plan_line(w.env, kDts[w.dt], w.mc, kCin[w.cin], w.cout, w.side, w.nhyp, 1, w.flags, w.ws, false, w.gn_G, w.tail_stats != 0);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s table | full ENV DTYPE\n", argv[0]);
    return 2;
}
