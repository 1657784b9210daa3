// stmmqr_diag.cpp -- the diagnostic prints of stmmqr_factorize_finish, one function each, called in the order they stand here.  The
// order matters for the three that read P.d_dbg: the block-0 and the pipeline printer clear its first 64 counters, so the pipeline
// printer sees what the block-0 printer left, and the timeline reads before either.  People diff these lines and the tests parse the
// "[early]" ones: the text is not to change.
#include "stmmqr_plan.h"

// STMMQR_DBG_EARLY: the fronts of a cut schedule that were not finished by their last scheduled panel (printed whatever finish goes on to report)
void stm_diag_early_fronts(const stmmqr_plan &P)
{
    if (!knobs::on(knobs::K_DBG_EARLY)) return;
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] < 0) continue;                  // factorized elsewhere
        const FrontNum &nm = P.h_fnum[f];
        const FrontSym &s = P.sch.fs[f];
        if (s.nsched < s.npanels && (!nm.done || nm.g < std::min(nm.fm, s.fn)))
            fprintf(stderr, "[early] front %ld fn %d fp %d fm %d fm_est %d fm_ub %d g %d rank %d done %d nsched %d npanels %d\n", f, s.fn, s.fp, nm.fm, s.fm_est,
                    s.fm_ub, nm.g, nm.rank, nm.done, s.nsched, s.npanels);
    }
}

// STMMQR_DUMPSTEPS=file (detail runs, diagnosis): one line per timeline step with what ran and how long it took.  pair_ms: the time
// of every event pair of the pass, P.evpairs[0 .. pair_ms.size())
void stm_diag_dump_steps(const stmmqr_plan &P, const std::vector<float> &pair_ms)
{
    FILE *dump = (!pair_ms.empty() && knobs::text(knobs::K_DUMPSTEPS)) ? fopen(knobs::text(knobs::K_DUMPSTEPS), "w") : nullptr;
    if (!dump) return;
    std::vector<float> st_panel, st_upd;
    if (!P.sch.gsteps.empty()) { st_panel.assign(P.sch.gsteps[0].size(), 0.f); st_upd.assign(P.sch.gsteps[0].size(), 0.f); }
    for (size_t q = 0; q < pair_ms.size(); q++) {
        if ((size_t)P.evpairs[q].step >= st_panel.size()) continue;
        if (P.evpairs[q].cat == 2) st_panel[(size_t)P.evpairs[q].step] += pair_ms[q];
        if (P.evpairs[q].cat == 3) st_upd[(size_t)P.evpairs[q].step] += pair_ms[q];
    }
    for (size_t t = 0; t < st_panel.size(); t++) {
        const Step &S = P.sch.gsteps[0][t];
        int maxrows = 0, pwg = 0;
        long tiles = 0;
        for (int i = 0; i < S.n_act; i++) {
            const FrontSym &fsym = P.sch.fs[P.sch.lists[S.act_off + i]];
            const int p = P.sch.lists[S.plist_off + i];
            maxrows = std::max(maxrows, stm_panel_rows_est(fsym, p));
            pwg += stm_use_ca(fsym, p, P.sch.plan_algo, P.sch.ca_min) ? stm_ca_slabs(fsym) : stm_tall_launches(fsym, p, P.sch.tall_min);
            tiles += (long)stm_upd_ncb(fsym, p) * stm_upd_nsl(fsym);
        }
        fprintf(dump, "%zu n_act %d maxrows %d nsub %d pwg %d nca_use %d maxcb %d maxsl %d split %d tiles %ld panel_us %.1f upd_us %.1f\n", t,
                S.n_act, maxrows, S.nsub, pwg, S.nca_use, S.maxcb, S.maxsl, S.split, tiles, 1e3 * st_panel[t], 1e3 * st_upd[t]);
    }
    fclose(dump);
}

// -DSTMMQR_STAMPS builds: wall-clock (100 MHz) timeline of panel 1 of the LAST front that ran one (the root), per column group
int stm_diag_panel_timeline(const stmmqr_plan &P, int dbg)
{
    if (!((dbg & 32) && knobs::on(knobs::K_TIMELINE))) return 0;
    std::vector<unsigned long long> hb(2048);
    HIPCHK(hipMemcpy(hb.data(), P.d_dbg.p, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull;
    for (int b = 0; b < 16; b++) if (hb[16 + 64 * b]) t0 = std::min(t0, hb[16 + 64 * b]);
    for (int b = 0; b < 16; b++) {
        const unsigned long long *q = &hb[16 + 64 * b];
        if (!q[0]) continue;
        fprintf(stderr, "[panel timeline] group %2d:", b);
        auto us = [&](int i) { return q[i] ? 0.01 * (double)(q[i] - t0) : -1.0; };
        fprintf(stderr, " start %.2f loaded %.2f |", us(0), us(1));
        for (int h = 0; h < 6 && q[2 + 3 * h]; h++) fprintf(stderr, " wait %.2f vload %.2f applied %.2f |", us(2 + 3 * h), us(3 + 3 * h), us(4 + 3 * h));
        fprintf(stderr, " cols");
        for (int j = 0; j < 8; j++) if (q[20 + j]) fprintf(stderr, " %.2f", us(20 + j));
        fprintf(stderr, " | published %.2f final %.2f\n", us(30), us(31));
    }
    return 0;
}

// STMMQR_DBG & 32768: where the time of a block-0 launch goes (slab 0); clears the counters
int stm_diag_block0_launch(const stmmqr_plan &P, int dbg)
{
    if (!(dbg & 32768)) return 0;
    unsigned long long hb[64];
    HIPCHK(hipMemcpy(hb, P.d_dbg.p, sizeof hb, hipMemcpyDeviceToHost));
    const double n = hb[56] ? 100.0 * (double)hb[56] : 1.0;
    fprintf(stderr, "[block-0 launch, slab 0, us] descriptors+loads issued %.2f  phase 1 %.2f  partials+ticket %.2f  wait %.2f  sums %.2f  T %.2f  W2 %.2f  phase 2 %.2f  (%llu)\n",
            hb[48] / n, hb[49] / n, hb[50] / n, hb[51] / n, hb[52] / n, hb[53] / n, hb[54] / n, hb[55] / n, hb[56]);
    HIPCHK(hipMemset(P.d_dbg.p, 0, sizeof hb));
    return 0;
}

// STMMQR_DBG & 48: the counters of the panel pipeline; clears them
int stm_diag_pipeline_counters(const stmmqr_plan &P, int dbg)
{
    if (!(dbg & 48)) return 0;
    unsigned long long hb[64];
    HIPCHK(hipMemcpy(hb, P.d_dbg.p, sizeof hb, hipMemcpyDeviceToHost));
    fprintf(stderr, "[pipeline panels by actual rows] <=128 %llu  <=256 %llu  <=512 %llu  <=1024 %llu  <=2048 %llu  <=4096 %llu  more %llu;  of the <=512: %llu with a row estimate > 512\n",
            hb[32], hb[33], hb[34], hb[35], hb[36], hb[37], hb[38], hb[39]);
    fprintf(stderr, "[k_upd_w workgroups] launched %llu  with work %llu\n", hb[40], hb[41]);
    fprintf(stderr, "[panel cycles, summed over workgroups] stage-in+apply %llu  columns %llu  write-back %llu  - %llu  gram %llu\n",
            hb[0], hb[1], hb[2], hb[3], hb[4]);
    fprintf(stderr, "[last group of the panel pipeline, cycles] load %llu  waits %llu  apply-loads %llu  applies %llu  factor %llu  gram %llu\n", hb[6],
            hb[7], hb[12], hb[8] + hb[11], hb[9], hb[10]);
    fprintf(stderr, "[panel workgroups] %llu  cycles %llu  100 MHz ticks %llu  => %.3f GHz, %.2f us per workgroup\n", hb[46], hb[44], hb[45],
            hb[45] ? 0.1 * (double)hb[44] / (double)hb[45] : 0.0, hb[46] ? 0.01 * (double)hb[45] / (double)hb[46] : 0.0);
    fprintf(stderr, "[Gram-based panels] panels %llu  refresh rounds %llu  slab workgroups %llu\n", hb[13], hb[14], hb[15]);
    HIPCHK(hipMemset(P.d_dbg.p, 0, sizeof hb));
    return 0;
}

// STMMQR_MEMDUMP: what the plan holds on the device (after P.stats.device_bytes is set)
void stm_diag_memdump(const stmmqr_plan &P)
{
    if (!knobs::on(knobs::K_MEMDUMP)) return;
    auto gb = [](const auto &b) { return (double)b.n * sizeof(*b.p) * 1e-9; };
    fprintf(stderr, "[stmmqr_hip] device memory (GB): fronts %.3f  contribution blocks %.3f  R+H %.3f  update workspaces %.3f + %.3f  "
                    "kept T %.3f  pair -Y %.3f  Sx/Ax/smap %.3f  per-column arrays %.3f  total %.3f  (recycle %d, kept fronts %d, maxstack %.3f)\n",
            gb(P.d_F), gb(P.d_C), gb(P.d_RH), gb(P.d_Wp), gb(P.d_Wp2), gb(P.d_Tall), gb(P.d_Ypend), gb(P.d_Sx) + gb(P.d_Ax) + gb(P.d_smap),
            gb(P.d_Stair) + gb(P.d_Tau) + gb(P.d_Hii) + gb(P.d_Cmap) + gb(P.d_Cursor) + gb(P.d_Rhoff) + gb(P.d_Rjrel) + gb(P.d_Sjrel),
            P.stats.device_bytes * 1e-9, (int)P.sch.recycle, (int)std::count(P.sch.kept.begin(), P.sch.kept.end(), (char)1), 8e-9 * (double)P.maxstack);
}
