// The library's tuning switches and test hooks as ONE table.  The integer hooks (brcnn_conv_set_tile*,
// brcnn_roi_align_set_exact) and brcnn_get_tuning / brcnn_set_tuning (policy.hip) are the only writers; the dispatchers
// read brcnn::g_policy.<member>.  A new switch is a member here (its default as the initialiser), a decoder line in
// policy.hip and, if it is a product default, a brcnn_tuning field.  Process-wide, unsynchronised (include/brcnn_hip.h).
#pragma once

namespace brcnn {

struct Policy {
    // ---- fp32 conv (conv_igemm.hip): brcnn_conv_set_tile(wm, nt)
    int use_dma = 1;                // LDS-DMA staged kernel for the FAST path; (-1, 0/1/2): register-staged / heuristic / always LDS-DMA
    int force_wm = 0, force_nt = 0; // tuning hooks (brcnn_conv_set_tile): 0 = heuristic
    int no_fast = 0;                // test hook (brcnn_conv_set_tile(-4, 0 / 1)): 1 = no straight-line read-out, no plain-layer set-up (every kernel, every dtype)
    int pp_f32_n128 = 1;            // tuning hook (brcnn_conv_set_tile(-3, 0 / 1 / 2)): the 256 x 128 eight-phase tile never / heuristic / forced
    int pp_f32_mode = 1;            // tuning hook (brcnn_conv_set_tile(-2, 0 / 1 / 2 / 128 / 256)): eight-phase fp32 kernel never / heuristic / forced (tile rows by the heuristic / 128 / 256)
    int f32_tile_sk = 1;            // tuning hook (brcnn_conv_set_tile(-5, 0 / 1 / 2)): persistent 64 x 64 launch never / heuristic / forced
    int f32_tile_sk_per_cu = 0;     // tuning hook ((-7, n)): workgroups per CU of the persistent launch, 0 = the occupancy query's
    // ---- fp32 Winograd F(2x2,3x3) (conv_winograd_f32.hip): brcnn_conv_set_tile(-11, n); read by the CALLER that prepares filters
    int f32_winograd = 1;           // (-11, 0 / 1): never / where the caller prepared the transformed filter; (-11, 2) returns it
    int f32_winograd_chunks = 1;    // tuning hook ((-11, 10 + n), n = 1 .. 8): transform + GEMM launch pairs per call
    // ... the single-layer route of the frozen backbone / neck 3x3 convs: brcnn_conv_set_tile(-14, n); read by
    // brcnn_winograd_layer_route (f32_winograd = 0 switches it off as well) and by brcnn_conv3x3_winograd_f32_layer
    int f32_winograd_layer = 1;     // (-14, 0 / 1 / 2): never / the measured rule (wino_layer_rule) / wherever the entry accepts the shape; (-14, 3) returns it
    int f32_winograd_gemm = 0;      // tuning hook ((-14, 20 + v)): GEMM tile of the layer entry, 0 = the measured rule (wino_gemm_rule), 1 = 64 x 128, 2 = 32 x 128, 3 = 64 x 64; (-14, 24) returns it
    // ... the persistent, balanced launch of the Winograd GEMM (both entries): brcnn_conv_set_tile(-16, n)
    int f32_winograd_sk = 1;        // (-16, 0 / 1 / 2): never / the measured rule (wino_persistent_rule) / wherever the schedule allows; (-16, 3) returns it
    int f32_winograd_sk_per_cu = 0; // tuning hook ((-16, 30 + n), n = 0 .. 8): workgroups per CU of the persistent launch at most, 0 = the occupancy query's; (-16, 39) returns it
    int f32_winograd_sk_wgs = 0;    // test hook ((-16, 1000 + n), n = 0 .. 2048): workgroups of the persistent launch at most (small maps then straddle tiles), 0 = no cap; (-16, 999) returns it
    int f32_winograd_ring = 0;      // tuning hook ((-16, 40 / 42 / 43)): LDS ring stages of the GEMM's K loop by the measured rule (wino_ring_rule) / 2 / 3; (-16, 49) returns it
    int f32_winograd_tower_gemm = 0;    // tuning hook ((-16, 20 + v)): GEMM tile of the tower entry, 0 = the measured rule (wino_tower_gemm_rule), 1 = 64 x 128, 3 = 64 x 64; (-16, 24) returns it

    // ---- 16-bit deformable conv (deform_conv_bf16.hip): brcnn_conv_set_tile(-13, n); read by brcnn_deform_conv_route
    int dcn_fused = 1;              // (-13, 0 / 1 / 2): im2col + GEMM always / the measured rule / fused wherever the kernel accepts the shape

    // ---- 16-bit conv (conv_igemm_bf16.hip, conv1x1_stream_bf16.hip): brcnn_conv_set_tile_bf16(mtnt)
    int bf16_tile = 0;              // tuning hook: 0 heuristic, 11 / 21 / 22 = MT NT (4 waves), 42 = 256x128 (8 waves)
    int bf16_il = 0;                // tuning hook (set_tile_bf16(-1 / -2)): spread the LDS-DMA pieces between the MFMA groups
    int sk_mode = 1;                // tuning hook (set_tile_bf16(-3 / -4 / -5)): 0 off, 1 heuristic, 2 wherever the tile count allows
    int sk_par = 0;                 // tuning hook (set_tile_bf16(-8 / -9 / -10)): split-K of few-tile launches off / heuristic / forced
    int pp_mode = 1;                // eight-phase 256 x 256 kernel (set_tile_bf16(-6 / -7)): 0 never, 1 heuristic
    int pp128_mode = 1;             // 256 x 128 two-group kernel (set_tile_bf16(-18 / -19)): 0 never, 1 heuristic
    int pp128_min_k = 4096;         // ... (-1000 - K): shortest K the heuristic takes
    int pp128_max_t88 = 128;        // ... (-2000 - n): N % 256 == 0 layers: 256 x 256 tiles from this count on (where pp_wins takes them)
    int sk_spin_limit = 1 << 24;    // ~5 s of polling; test hook -11 / -12: 256 polls and heads that do not publish / back
    int sk_drop_publish = 0;
    int stream_mode = 1;            // persistent short-K 1x1 kernel (set_tile_bf16(-15 / -16 / -17)): never / heuristic / wherever the shape allows

    // ---- 16-bit weight gradient (conv_wgrad_bf16.hip, conv_wgrad_pp_bf16.hip): brcnn_conv_set_tile_wgrad_bf16(wt)
    int wgrad_bf16_tile = 0;        // tuning hook: 0 heuristic, 1 = 64x64, 2 = 128x128, 4 = 256x256 (16 waves)
    int wgrad_slabs = 1;            // tuning hook (brcnn_conv_set_tile_wgrad_bf16(10 / 11)): 0 atomics, 1 slabs + second stage
    int wgrad_slot_pct = 75;        // ... (2000 + n): n percent of a generation of workgroups per launch (75: the launches share the device with the main stream; same-box A/B 19.92 -> 19.75 ms per step, 50 % level, 35 % +0.9 ms)
    int wgrad_slot_pct_big = 75;    // ... (3000 + n): the same for launches of more than 2^17 reduction rows on the 256 x 256 tile
    int wgrad_two_pass = 24;        // ... (100 + n): more than n slices per tile -> the second stage runs as two passes
    int wgrad_pp_mode = 1;          // tuning hook (brcnn_conv_set_tile_wgrad_bf16(20 / 21 / 22)): never / heuristic / wherever the shape allows
    int wgrad_pp_slot_pct = 75;     // ... (4000 + n): n percent of the CUs per launch (the launches share the device with the main stream)
    int wgrad_pp_two_pass = 24;     // ... (5000 + n): two reduce passes above n slices
    int wgrad_pp_fuse = 0;          // ... (30 / 31): slab reduction as separate launches / inside the producing launch.  Measured (r04_notes.md):
                                    // the in-launch form costs ~70 us per launch (one workgroup pulling 1-3 MB is latency-bound) -> off

    // ---- RoI (roi_align.hip): brcnn_roi_align_set_exact(exact)
    int roi_exact = 0;              // 1: exact sample-order kernel (bit-identical to the reference's CPU order)
    int roi_stream_c = 3;           // footprint kernel: bit 0 column streaming over the bin row's patch (else the per-bin loop), bit 1 XCD-contiguous rows
    int roi_prep = 0;               // ... (30 / 31): prepared-record form off / on where the caller provides its scratch.  OFF: measured
                                    // slower below 1000 RoIs / image (profiles/r05_notes.md)
    int roi_rpw = 0;                // tuning hook (set_exact(10 / 11 / 17)): rows per wave by the heuristic / 1 / all (stored 0 / 11 / 17)
    int roi_order = 1;              // ... (20 / 21 / 22): never / where a workspace is given and the RoI count pays for the sort / always
    int roi_gather_chunks = -1;     // tuning hook (brcnn_roi_align_set_exact(40 + n)): -1 heuristic, n chunks per coarse tile
};
extern Policy g_policy;

// what the hooks report; the launch sites increment them
struct Counters {
    int f32_tile_sk_launches = 0;   // persistent launches so far (brcnn_conv_set_tile(-6, 0) reports it)
    int f32_tile_sk_wgs = 0;        // ... and the workgroups of the last one ((-6, 1))
    int wgrad_pp_launches = 0;      // launches taken so far (tests: hook 29 returns and clears it)
    // ---- which route a launch took (tests): brcnn_conv_set_tile(-9, n) returns counter n and clears it, (-9, -1) clears all of
    // them.  Counts wrap inside the positive ints (brcnn::count); the launch sites count after the launch
    int pp_f32_launches = 0;        // n = 0: fp32 eight-phase launches (conv_pp_f32.hip)
    int pp_f32_rows = 0;            // n = 1: ... tile rows of the last one (256 / 128)
    int pp_f32_cols = 0;            // n = 2: ... and its tile columns (256 / 128)
    int pp_bf16_launches = 0;       // n = 3: 256 x 256 eight-phase 16-bit launches (conv_pp_bf16.hip)
    int pp128_bf16_launches = 0;    // n = 4: 256 x 128 two-group 16-bit launches (conv_pp128_bf16.hip)
    int stream1x1_launches = 0;     // n = 5: persistent short-K 1x1 launches (conv1x1_stream_bf16.hip)
    int sk_chain_fills = 0;         // n = 6: launches planned as chained stream-K (sk_plan -> sk_table)
    int sk_par_fills = 0;           // n = 7: launches planned as split-K (sk_plan -> sk_table_par)
    int sk_last_wgs = 0;            // n = 8: workgroups of the last of either (the fp32 64 x 64 persistent launch keeps f32_tile_sk_*)
    int bf16_tile_launches = 0;     // n = 9: launches of the two-buffer / ring 16-bit tile kernel (conv_igemm_bf16.hip launch2)
    int bf16_tile_rows = 0;         // n = 10: ... the last one's tile rows,
    int bf16_tile_cols = 0;         // n = 11: tile columns,
    int bf16_tile_waves = 0;        // n = 12: waves per workgroup
    int bf16_tile_stages = 0;       // n = 13: and LDS ring stages
    int wgrad_bf16_tile_launches = 0;   // n = 14: launches of the tile kernel of conv_wgrad_bf16.hip (not the eight-phase one)
    int wgrad_bf16_last_tile = 0;       // n = 15: the tile code (1 / 2 / 4) of the last one
    // brcnn_conv_set_tile(-12, 0 / 1): return and clear ((-9, -1) clears them too)
    int f32_winograd_launches = 0;      // (-12, 0): calls of brcnn_conv3x3_winograd_f32_multi that launched
    int f32_winograd_tiles = 0;         // (-12, 1): 2x2 output tiles of the last one
    // brcnn_conv_set_tile(-14, 10 / 11): return and clear ((-9, -1) clears them too)
    int f32_winograd_layer_launches = 0;    // (-14, 10): calls of brcnn_conv3x3_winograd_f32_layer that launched (the tower's are not in it)
    int f32_winograd_layer_variant = 0;     // (-14, 11): GEMM tile of the last one (1 = 64 x 128, 2 = 32 x 128, 3 = 64 x 64)
    // brcnn_conv_set_tile(-16, 10 .. 13): return and clear ((-9, -1) clears them too)
    int f32_winograd_sk_launches = 0;       // (-16, 10): persistent Winograd GEMM launches (either entry; a call of n launch pairs counts up to n)
    int f32_winograd_sk_last_wgs = 0;       // (-16, 11): workgroups of the last one
    int f32_winograd_tower_variant = 0;     // (-16, 12): GEMM tile of the last tower call (1 = 64 x 128, 3 = 64 x 64)
    int f32_winograd_last_ring = 0;         // (-16, 13): LDS ring stages of the last Winograd GEMM launch (2 / 3)
    // brcnn_conv_set_tile(-13, 10 / 11): return and clear ((-9, -1) clears them too)
    int dcn_fused_launches = 0;         // (-13, 10): launches of the fused deformable conv (deform_conv_bf16.hip), every entry
    int dcn_im2col_launches = 0;        // (-13, 11): launches of the deformable im2col kernels (deform.hip), every entry
    // brcnn_roi_align_set_exact(60 .. 63): return and clear
    int roi_ordered_launches = 0;   // 60: RoI forward launches that visited the RoIs in band order
    int roi_prepared_launches = 0;  // 61: RoI forward launches in the prepared-record form
    int roi_gather_chunked = 0;     // 62: RoI gradient gathers that ran chunked (partials + chunk sum)
    int roi_gather_last_ch = 0;     // 63: chunks per coarse tile of the last of them
};
extern Counters g_counters;
inline void count(int& c) { c = (c + 1) & 0x7fffffff; }     // (a long run must not overflow a signed int)

// The measured rules of the Winograd single-layer route (policy.hip; host only, no launch): does a frozen 3x3 stride-1 layer
// of `tiles` 2x2 output tiles gain from the Winograd form (1) or stay on the direct kernels (0); and the GEMM tile of such a
// launch (1 / 2 / 3, or the forced one)
int wino_layer_rule(int tiles, int cin, int cout);
int wino_gemm_rule(int tiles, int cout);
int wino_gemm_variant(int tiles, int cout);
// ... of the persistent launch of the Winograd GEMM: does a launch of `workgroup_tiles` GEMM tiles of `units` xi planes each
// gain from `per_cu` balanced workgroups on each of `cus` CUs (1) or stay one workgroup per tile (0); and the tower's tile
int wino_persistent_rule(int workgroup_tiles, int units, int cus, int per_cu);
int wino_tower_gemm_rule(int tiles, int cout);
int wino_ring_rule(int workgroup_tiles, int cin);       // LDS ring stages (2 / 3) of a GEMM launch

}  // namespace brcnn
