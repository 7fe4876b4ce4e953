// The policy table (policy.h) and its two interfaces: the integer hooks decode their codes into members of g_policy,
// brcnn_get_tuning / brcnn_set_tuning copy the public fields (include/brcnn_hip.h: brcnn_tuning).  Host code only.
#include "common.h"
#include "policy.h"

__attribute__((require_constant_initialization)) brcnn::Policy brcnn::g_policy;
__attribute__((require_constant_initialization)) brcnn::Counters brcnn::g_counters;
using brcnn::g_counters, brcnn::g_policy;

BRCNN_API int brcnn_conv_set_tile(int wm, int nt) {
    if (wm == -1) { g_policy.use_dma = nt; return 0; }   // (-1, 0/1/2): register-staged / heuristic / always LDS-DMA
    if (wm == -3) { if (nt < 0 || nt > 2) return BRCNN_EINVAL; g_policy.pp_f32_n128 = nt; return 0; }
    if (wm == -4) { if (nt != 0 && nt != 1) return BRCNN_EINVAL; g_policy.no_fast = nt; return 0; }
    if (wm == -5) { if (nt < 0 || nt > 2) return BRCNN_EINVAL; g_policy.f32_tile_sk = nt; return 0; }
    if (wm == -7) { if (nt < 0 || nt > 8) return BRCNN_EINVAL; g_policy.f32_tile_sk_per_cu = nt; return 0; }
    // (-6, 0): persistent 64 x 64 launches so far (>= 0), (-6, 1): workgroups of the last one
    if (wm == -6) return nt == 0 ? g_counters.f32_tile_sk_launches : nt == 1 ? g_counters.f32_tile_sk_wgs : BRCNN_EINVAL;
    // (-9, n): which route the launches took (policy.h Counters lists n = 0 .. 15): returns counter n and clears it,
    // (-9, -1) clears them all
    if (wm == -9) {
        int* const c[] = {&g_counters.pp_f32_launches, &g_counters.pp_f32_rows, &g_counters.pp_f32_cols, &g_counters.pp_bf16_launches,
                          &g_counters.pp128_bf16_launches, &g_counters.stream1x1_launches, &g_counters.sk_chain_fills,
                          &g_counters.sk_par_fills, &g_counters.sk_last_wgs, &g_counters.bf16_tile_launches, &g_counters.bf16_tile_rows,
                          &g_counters.bf16_tile_cols, &g_counters.bf16_tile_waves, &g_counters.bf16_tile_stages,
                          &g_counters.wgrad_bf16_tile_launches, &g_counters.wgrad_bf16_last_tile};
        const int count = (int)(sizeof(c) / sizeof(c[0]));
        if (nt < -1 || nt >= count) return BRCNN_EINVAL;
        if (nt == -1) {
            for (int* q : c) *q = 0;
            g_counters.f32_winograd_launches = g_counters.f32_winograd_tiles = 0;
            g_counters.dcn_fused_launches = g_counters.dcn_im2col_launches = 0;
            g_counters.f32_winograd_layer_launches = g_counters.f32_winograd_layer_variant = 0;
            g_counters.f32_winograd_sk_launches = g_counters.f32_winograd_sk_last_wgs = g_counters.f32_winograd_tower_variant = 0;
            g_counters.f32_winograd_last_ring = 0;
            return 0;
        }
        const int n = *c[nt];
        *c[nt] = 0;
        return n;
    }
    // Winograd F(2x2,3x3) for the fp32 3x3 layers whose caller prepared the filter: (-11, 0 / 1) never / yes, (-11, 2) RETURNS
    // the setting (the caller decides: the entry point itself never falls back), (-11, 10 + n): n launch pairs per call
    if (wm == -11) {
        if (nt == 0 || nt == 1) { g_policy.f32_winograd = nt; return 0; }
        if (nt == 2) return g_policy.f32_winograd;
        if (nt >= 11 && nt <= 18) { g_policy.f32_winograd_chunks = nt - 10; return 0; }
        return BRCNN_EINVAL;
    }
    // (-12, 0): Winograd calls so far, (-12, 1): tiles of the last one; return and clear
    if (wm == -12) {
        if (nt != 0 && nt != 1) return BRCNN_EINVAL;
        int& c = nt == 0 ? g_counters.f32_winograd_launches : g_counters.f32_winograd_tiles;
        const int n = c;
        c = 0;
        return n;
    }
    // deformable conv route (brcnn_deform_conv_route): (-13, 0 / 1 / 2) im2col + GEMM always / by the measured rule / the
    // fused kernel wherever it accepts the shape; (-13, 3) RETURNS the setting; (-13, 10 / 11) return and clear the
    // launches of the fused kernel / of the im2col kernels
    if (wm == -13) {
        if (nt >= 0 && nt <= 2) { g_policy.dcn_fused = nt; return 0; }
        if (nt == 3) return g_policy.dcn_fused;
        if (nt != 10 && nt != 11) return BRCNN_EINVAL;
        int& c = nt == 10 ? g_counters.dcn_fused_launches : g_counters.dcn_im2col_launches;
        const int n = c;
        c = 0;
        return n;
    }
    // Winograd single-layer route (brcnn_winograd_layer_route): (-14, 0 / 1 / 2) never / by the measured rule / wherever the
    // entry accepts the shape, (-14, 3) RETURNS the setting; (-14, 10 / 11) return and clear the launches of the layer entry /
    // the GEMM tile of the last one; (-14, 20 + v): GEMM tile by the rule (v = 0) or forced (1 = 64 x 128, 2 = 32 x 128,
    // 3 = 64 x 64), (-14, 24) RETURNS that setting
    if (wm == -14) {
        if (nt >= 0 && nt <= 2) { g_policy.f32_winograd_layer = nt; return 0; }
        if (nt == 3) return g_policy.f32_winograd_layer;
        if (nt >= 20 && nt <= 23) { g_policy.f32_winograd_gemm = nt - 20; return 0; }
        if (nt == 24) return g_policy.f32_winograd_gemm;
        if (nt != 10 && nt != 11) return BRCNN_EINVAL;
        int& c = nt == 10 ? g_counters.f32_winograd_layer_launches : g_counters.f32_winograd_layer_variant;
        const int n = c;
        c = 0;
        return n;
    }
    // persistent launch of the Winograd GEMM: (-16, 0 / 1 / 2) never / by the measured rule / wherever the schedule allows,
    // (-16, 3) RETURNS the setting; (-16, 10 .. 13) return and clear the persistent launches / the workgroups of the last
    // one / the GEMM tile of the last tower call / the LDS ring stages of the last GEMM launch; (-16, 40 / 42 / 43): ring
    // stages by the rule / 2 / 3, (-16, 49) RETURNS it; (-16, 20 + v): the tower's GEMM tile by the rule (v = 0) or forced (1 =
    // 64 x 128, 3 = 64 x 64), (-16, 24) RETURNS it; (-16, 30 + n), n = 0 .. 8: at most n workgroups per CU (0: the occupancy
    // query's), (-16, 39) RETURNS it; (-16, 1000 + n), n = 0 .. 2048: at most n workgroups in all (0: no cap), (-16, 999)
    // RETURNS it
    if (wm == -16) {
        if (nt >= 0 && nt <= 2) { g_policy.f32_winograd_sk = nt; return 0; }
        if (nt == 3) return g_policy.f32_winograd_sk;
        if (nt == 20 || nt == 21 || nt == 23) { g_policy.f32_winograd_tower_gemm = nt - 20; return 0; }
        if (nt == 24) return g_policy.f32_winograd_tower_gemm;
        if (nt >= 30 && nt <= 38) { g_policy.f32_winograd_sk_per_cu = nt - 30; return 0; }
        if (nt == 39) return g_policy.f32_winograd_sk_per_cu;
        if (nt == 40 || nt == 42 || nt == 43) { g_policy.f32_winograd_ring = nt - 40; return 0; }
        if (nt == 49) return g_policy.f32_winograd_ring;
        if (nt >= 1000 && nt <= 1000 + 2048) { g_policy.f32_winograd_sk_wgs = nt - 1000; return 0; }
        if (nt == 999) return g_policy.f32_winograd_sk_wgs;
        if (nt < 10 || nt > 13) return BRCNN_EINVAL;
        int& c = nt == 10 ? g_counters.f32_winograd_sk_launches : nt == 11 ? g_counters.f32_winograd_sk_last_wgs
                 : nt == 12 ? g_counters.f32_winograd_tower_variant : g_counters.f32_winograd_last_ring;
        const int n = c;
        c = 0;
        return n;
    }
    if (wm == -2) { if (nt != 0 && nt != 1 && nt != 2 && nt != 128 && nt != 256) return BRCNN_EINVAL; g_policy.pp_f32_mode = nt; return 0; }
    if ((wm != 0 && wm != 1 && wm != 2 && wm != 4) || nt < 0 || nt > 2) return BRCNN_EINVAL;
    g_policy.force_wm = wm;
    g_policy.force_nt = nt;
    return 0;
}

// ---- the Winograd single-layer route: the measured rules (profiles/f32_winograd_layers.txt: MI355X, the production launch
// of each layer against the Winograd entry per GEMM tile, batch 8 and batch 1 of the flagship pass's maps and probes
// between them; a point wins where the gain exceeds the spread of the direct rounds)
int brcnn::wino_gemm_rule(int tiles, int cout) {
    // 64 x 64 was the fastest tile on every row of the table, from 616 to 33 600 tiles and 128 to 512 channels (the 32 x 32
    // wave tiles run four waves per SIMD where 64 x 128 runs two; at 8 400 tiles 243 us against 299 us)
    (void)tiles; (void)cout;
    return 3;
}

int brcnn::wino_layer_rule(int tiles, int cin, int cout) {
    // per channel class the threshold lies midway between the nearest losing (or not proven) and the nearest winning
    // measured tile count; classes that were not measured stay on the direct kernels
    if (cin != cout) return 0;
    // 128 -> 128 (stage-2 conv2) is NOT wired although it wins from about 3 200 tiles on (2 184: -14 us of 49; 4 200: +4 us of
    // 69; 33 600: +62 us of 326, three launches per pass): with it the flagship pass's detections keep their values to
    // round-off, but two of them whose scores are 4e-7 apart change places in the result list (profiles/r09_notes.md), and
    // the pass has to return what it returned before
    if (cin == 256) return tiles >= 5250;       // 4 200: +12 us of 177 inside the spread (18); 6 300: +107 us of 281, 8 400: +65 us of 308
    if (cin == 512) return tiles >= 444;        // 273: -62 us of 112; 616: +3 us of 180 (spread 3), 2 184: +45 us of 344
    return 0;
}

int brcnn::wino_gemm_variant(int tiles, int cout) {
    return g_policy.f32_winograd_gemm ? g_policy.f32_winograd_gemm : wino_gemm_rule(tiles, cout);
}

// ---- the persistent launch of the Winograd GEMM: the measured rules (profiles/f32_winograd_persistent.txt: MI355X, 256
// CUs, transform + GEMM per shape, plain against forced persistent, 7 alternating rounds of 10 launches; a class takes a
// form where its gain exceeds the spread of the plain rounds).  `per_cu` is what the launch would run: the resident count,
// or floor(workgroup_tiles / cus), one at least, where the launch has fewer GEMM tiles than that (conv_winograd_f32.hip:
// wino_plan).  The thresholds are the midpoints between the nearest losing and the nearest winning measured tile count of a
// class, as tiles per CU (x / 256).
int brcnn::wino_persistent_rule(int workgroup_tiles, int units, int cus, int per_cu) {
    if (workgroup_tiles <= 0 || units < 16 || cus <= 0 || per_cu <= 0) return 0;
    const long long t256 = (long long)workgroup_tiles * 256;
    // ONE balanced workgroup per CU, 1.03 - 1.25 chains each, where the plain launch leaves a few CUs with two whole chains:
    // 264 GEMM tiles 164 -> 124 us, 280 (512 channels) 297 -> 219 us, 320 166 -> 143 us (spreads 6 - 8 us); at 396 the
    // second workgroup is on more than half of the CUs and nearly free there: 174 -> 175 us
    if (per_cu == 1) return workgroup_tiles >= cus && t256 < 358LL * cus;
    // TWO per CU, 2.06 chains each, where the plain launch puts a third workgroup on a few CUs: 528 GEMM tiles 241 -> 200 us
    // (spread 13 us).  512 is two whole chains per CU either way (182 -> 183 us), and at 640 the plain launch's third
    // workgroups are on half of the CUs: 252 -> 239 us, inside the spread of 20 us
    if (per_cu == 2) return t256 >= 520LL * cus && t256 < 584LL * cus;
    // more GEMM tiles than places (33 600 tiles: 2 100 GEMM tiles on four per CU, 793 -> 775 us inside the spread of 59 us,
    // -73 us on two per CU) and the tower (1 406: 1006 -> 991 us, a gain the size of the persistent rounds' own spread; its
    // 64 x 64 tile -95 us): plain.  Three and more whole chains per CU were not measured
    return 0;
}

// LDS ring stages of the GEMM's K loop.  Three stages lost 3 - 10 us on every plain launch of the table but the 33 600-tile
// one (+21 us inside its spread of 59 us) and moved the persistent ones by -3 .. +6 us, inside or at the edge of their
// spreads: two everywhere
int brcnn::wino_ring_rule(int workgroup_tiles, int cin) {
    (void)workgroup_tiles; (void)cin;
    return 2;
}

// the tower's GEMM tile: 64 x 128 (1) or 64 x 64 (3).  64 x 64 measured 973 against 1006 us, inside its own spread of 61 us
int brcnn::wino_tower_gemm_rule(int tiles, int cout) {
    (void)tiles; (void)cout;
    return 1;
}

// host arithmetic only (tests, tools): brcnn::wino_persistent_rule
BRCNN_API int brcnn_winograd_persistent_rule(int workgroup_tiles, int units, int cus, int per_cu) {
    return brcnn::wino_persistent_rule(workgroup_tiles, units, cus, per_cu);
}

// 1: the frozen fp32 conv layer of this form and size runs brcnn_conv3x3_winograd_f32_layer, 0: the launches it ran before.
// Host only, launches nothing.  0 for anything but 3x3, stride 1, pad 1, dilation 1, groups 1, Cin % 32 == 0, Cout % 64 == 0,
// fp32; 0 while the library's Winograd switch ((-11, 0)) or the route ((-14, 0)) is off; (-14, 2): 1 for every such layer;
// (-14, 1), the default: brcnn::wino_layer_rule.
BRCNN_API int brcnn_winograd_layer_route(int tiles, int cin, int cout, int kh, int kw, int stride, int pad, int dilation,
                                         int groups, int dtype) {
    if (tiles <= 0 || cin <= 0 || cout <= 0 || kh != 3 || kw != 3 || stride != 1 || pad != 1 || dilation != 1 || groups != 1 ||
        (cin % 32) || (cout % 64) || dtype != BRCNN_DT_F32 || (long long)cout * cin * 64 >= 0x7fffffffLL)
        return 0;
    if (!g_policy.f32_winograd || !g_policy.f32_winograd_layer) return 0;
    if (g_policy.f32_winograd_layer == 2) return 1;
    return brcnn::wino_layer_rule(tiles, cin, cout);
}

// the GEMM tile brcnn_conv3x3_winograd_f32_layer would launch for (tiles, cout): 1 / 2 / 3 (tools, tests)
BRCNN_API int brcnn_winograd_layer_gemm_variant(int tiles, int cout) { return brcnn::wino_gemm_variant(tiles, cout); }

BRCNN_API int brcnn_conv_set_tile_bf16(int mtnt) {
    if (mtnt == -1 || mtnt == -2) { g_policy.bf16_il = (mtnt == -1); return 0; }
    if (mtnt <= -3 && mtnt >= -5) { g_policy.sk_mode = -3 - mtnt; return 0; }       // stream-K: -3 off, -4 heuristic, -5 forced
    if (mtnt <= -8 && mtnt >= -10) { g_policy.sk_par = -8 - mtnt; return 0; }       // split-K of few-tile launches: -8 off, -9 heuristic, -10 forced
    if (mtnt == -6 || mtnt == -7) { g_policy.pp_mode = mtnt == -7; return 0; }      // eight-phase kernel: -6 never, -7 heuristic
    if (mtnt == -18 || mtnt == -19) { g_policy.pp128_mode = mtnt == -19; return 0; }   // 256 x 128 two-group kernel: -18 never, -19 heuristic
    if (mtnt <= -1000 && mtnt > -2000) { g_policy.pp128_min_k = -1000 - mtnt; return 0; }      // ... its shortest K (-1000 - K)
    if (mtnt <= -2000 && mtnt > -3000) { g_policy.pp128_max_t88 = -2000 - mtnt; return 0; }    // ... 256 x 256 tiles from this count on
    if (mtnt <= -15 && mtnt >= -17) { g_policy.stream_mode = -15 - mtnt; return 0; }      // persistent short-K 1x1 kernel never / heuristic / forced
    // test hook: -11 = the K heads of the following stream-K launches do not publish and the tails give up after 256
    // polls (a lost hand-over, to exercise BRCNN_EHANDOVER); -12 = back to normal
    if (mtnt == -11 || mtnt == -12) { g_policy.sk_drop_publish = mtnt == -11; g_policy.sk_spin_limit = mtnt == -11 ? 256 : 1 << 24; return 0; }
    const int ok[] = {0, 11, 21, 22, 42, 82, 81, 164, 342, 382, 3164, 322, 482, 381, 2244, 2144, 8844, 8842};
    bool found = false;
    for (int v : ok) found |= (v == mtnt);
    if (!found) return BRCNN_EINVAL;
    g_policy.bf16_tile = mtnt;
    return 0;
}

BRCNN_API int brcnn_conv_set_tile_wgrad_bf16(int wt) {
    if (wt == 10 || wt == 11) { g_policy.wgrad_slabs = wt - 10; return 0; }      // reduction over the M slices: atomics / slabs
    if (wt >= 100 && wt < 1100) { g_policy.wgrad_two_pass = wt - 100; return 0; }
    if (wt >= 2010 && wt <= 2400) { g_policy.wgrad_slot_pct = wt - 2000; return 0; }
    if (wt >= 3010 && wt <= 3400) { g_policy.wgrad_slot_pct_big = wt - 3000; return 0; }
    // eight-phase kernel (conv_wgrad_pp_bf16.hip): 20 never / 21 heuristic / 22 wherever the shape allows; 4000 + n: n
    // percent of the CUs per launch; 5000 + n: two reduce passes above n slices; 29: RETURNS the number of launches the
    // eight-phase kernel took since the last query (tests); 30 / 31: its slab reduction as separate launches / inside the
    // producing launch
    if (wt >= 20 && wt <= 22) { g_policy.wgrad_pp_mode = wt - 20; return 0; }
    if (wt == 29) { const int n = g_counters.wgrad_pp_launches; g_counters.wgrad_pp_launches = 0; return n; }
    if (wt == 30 || wt == 31) { g_policy.wgrad_pp_fuse = wt - 30; return 0; }
    if (wt >= 4010 && wt <= 4400) { g_policy.wgrad_pp_slot_pct = wt - 4000; return 0; }
    if (wt >= 5001 && wt <= 5999) { g_policy.wgrad_pp_two_pass = wt - 5000; return 0; }
    if (wt < 0 || wt == 3 || wt > 4) return BRCNN_EINVAL;
    g_policy.wgrad_bf16_tile = wt;
    return 0;
}

BRCNN_API int brcnn_roi_align_set_exact(int exact) {
    // 0: footprint kernel (column streaming, XCD-contiguous bin rows), 1: exact sample order, 2: footprint kernel with
    // the per-bin loop and round-robin rows (the r02 form), 3: column streaming with round-robin rows
    // 10 / 11 / 17: bin rows per wavefront by the heuristic / one / all seven; 20 / 21 / 22: RoI visiting order off / by the heuristic / forced
    if (exact == 10 || exact == 11 || exact == 17) { g_policy.roi_rpw = exact == 10 ? 0 : exact; return 0; }
    if (exact >= 20 && exact <= 22) { g_policy.roi_order = exact - 20; return 0; }
    if (exact == 30 || exact == 31) { g_policy.roi_prep = exact - 30; return 0; }
    if (exact >= 39 && exact <= 56) { g_policy.roi_gather_chunks = exact - 40; return 0; }    // 39: heuristic, 40 / 41: off, 42..56: chunks per coarse tile
    // 60 .. 63 (tests): RETURN and clear -- forward launches that took the band order / the prepared-record form, gradient
    // gathers that ran chunked / the chunks per coarse tile of the last of them
    if (exact >= 60 && exact <= 63) {
        int* const c[] = {&g_counters.roi_ordered_launches, &g_counters.roi_prepared_launches, &g_counters.roi_gather_chunked,
                          &g_counters.roi_gather_last_ch};
        const int n = *c[exact - 60];
        *c[exact - 60] = 0;
        return n;
    }
    g_policy.roi_exact = exact == 1 ? 1 : 0;
    g_policy.roi_stream_c = exact == 2 ? 0 : exact == 3 ? 1 : 3;
    return 0;
}

BRCNN_API int brcnn_get_tuning(brcnn_tuning* t) {
    if (!t || t->size != (int)sizeof(brcnn_tuning)) return BRCNN_EINVAL;
    t->conv_stream_k = g_policy.sk_mode;
    t->conv_split_k = g_policy.sk_par;
    t->conv_eight_phase_16bit = g_policy.pp_mode;
    t->conv_persistent_1x1 = g_policy.stream_mode;
    t->conv_eight_phase_f32 = g_policy.pp_f32_mode;
    t->wgrad_slab_reduction = g_policy.wgrad_slabs;
    t->wgrad_eight_phase = g_policy.wgrad_pp_mode;
    t->wgrad_reduce_in_launch = g_policy.wgrad_pp_fuse;
    t->wgrad_generation_percent = g_policy.wgrad_slot_pct;
    t->wgrad_eight_phase_cu_percent = g_policy.wgrad_pp_slot_pct;
    t->roi_exact_order = g_policy.roi_exact;
    t->roi_rows_per_wave = g_policy.roi_rpw == 0 ? 0 : (g_policy.roi_rpw == 17 ? 7 : 1);
    t->roi_visit_order = g_policy.roi_order;
    t->roi_prepared_records = g_policy.roi_prep;
    return 0;
}

BRCNN_API int brcnn_set_tuning(const brcnn_tuning* t) {
    if (!t || t->size != (int)sizeof(brcnn_tuning)) return BRCNN_EINVAL;
    auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
    if (!in(t->conv_stream_k, 0, 2) || !in(t->conv_split_k, 0, 2) || !in(t->conv_eight_phase_16bit, 0, 1) ||
        !in(t->conv_persistent_1x1, 0, 2) ||
        !(in(t->conv_eight_phase_f32, 0, 2) || t->conv_eight_phase_f32 == 128 || t->conv_eight_phase_f32 == 256) ||
        !in(t->wgrad_slab_reduction, 0, 1) || !in(t->wgrad_eight_phase, 0, 2) || !in(t->wgrad_reduce_in_launch, 0, 1) ||
        !in(t->wgrad_generation_percent, 10, 400) || !in(t->wgrad_eight_phase_cu_percent, 10, 400) ||
        !in(t->roi_exact_order, 0, 1) || !(t->roi_rows_per_wave == 0 || t->roi_rows_per_wave == 1 || t->roi_rows_per_wave == 7) ||
        !in(t->roi_visit_order, 0, 2) || !in(t->roi_prepared_records, 0, 1))
        return BRCNN_EINVAL;
    g_policy.sk_mode = t->conv_stream_k;
    g_policy.sk_par = t->conv_split_k;
    g_policy.pp_mode = t->conv_eight_phase_16bit;
    g_policy.stream_mode = t->conv_persistent_1x1;
    g_policy.pp_f32_mode = t->conv_eight_phase_f32;
    g_policy.wgrad_slabs = t->wgrad_slab_reduction;
    g_policy.wgrad_pp_mode = t->wgrad_eight_phase;
    g_policy.wgrad_pp_fuse = t->wgrad_reduce_in_launch;
    g_policy.wgrad_slot_pct = t->wgrad_generation_percent;
    g_policy.wgrad_pp_slot_pct = t->wgrad_eight_phase_cu_percent;
    g_policy.roi_exact = t->roi_exact_order;
    g_policy.roi_stream_c = 3;      // as brcnn_roi_align_set_exact(0 / 1): the struct selects the default footprint form
    g_policy.roi_rpw = t->roi_rows_per_wave == 0 ? 0 : (t->roi_rows_per_wave == 7 ? 17 : 11);
    g_policy.roi_order = t->roi_visit_order;
    g_policy.roi_prep = t->roi_prepared_records;
    return 0;
}
