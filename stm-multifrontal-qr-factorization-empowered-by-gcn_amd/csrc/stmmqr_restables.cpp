// stmmqr_restables.cpp -- see stmmqr_restables.h
#include "stmmqr_restables.h"

#include <algorithm>
#include <climits>

namespace restab {
LevelTables level_tables(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists, int qt4_doubles)
{
    LevelTables T;
    T.lds_qa.assign(LV.size(), 0);
    T.lds_qa_all.assign(LV.size(), 0);
    T.lds_rs.assign(LV.size(), 0);
    T.lds_rt.assign(LV.size(), 0);
    T.qbig.assign(LV.size(), QbLevel());
    T.rtbig.assign(LV.size(), RtLevel());
    long xf = 1, dq = 1, wq = 1;
    for (size_t l = 0; l < LV.size(); l++) {
        long xo = 0, dqo = 0, wo = 0, lco = 0;
        T.qbig[l].off = (int)T.qb.size();
        T.rtbig[l].off = (int)T.rtb.size();
        T.qbig[l].t4i_off = (int)T.t4items.size();
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = lists[(size_t)(LV[l].all_off + q)];
            const FrontSym &s = fs[(size_t)f];
            const int need = (int)std::min(stm_lds_qapply(s.fm_ub, s.fn), (long)INT_MAX);
            T.lds_rt[l] = std::max(T.lds_rt[l], (int)std::min(stm_lds_rtsolve(s.fp, s.fm_ub, s.fn), (long)INT_MAX));
            T.lds_qa_all[l] = std::max(T.lds_qa_all[l], need);
            if (s.rtbig) {
                RtLevel &R = T.rtbig[l];
                RtDesc d;
                d.f = f; d.lcoff = (int)lco;
                T.rtb.push_back(d);
                lco += s.fp;
                const int rmax = std::min(s.fp, s.fm_ub);
                R.n++; R.max_steps = std::max(R.max_steps, (rmax + 31) / 32);
                R.max_nslab = std::max(R.max_nslab, std::max(1, (rmax + s.fn - s.fp + STM_RTB_COLS - 1) / STM_RTB_COLS));
            } else {
                T.rtbig[l].lds_small = std::max(T.rtbig[l].lds_small, (int)stm_lds_rtsolve(s.fp, s.fm_ub, s.fn));
            }
            if (s.qbig) {
                QbDesc d;
                d.f = f; d.xoff = (int)xo; d.dqoff = (int)dqo; d.wqoff = (int)wo; d.nslab = (s.fm_ub + STM_QB_ROWS - 1) / STM_QB_ROWS; d.np_live = s.npanels;
                T.qb.push_back(d);
                const int ngr = (s.npanels + 3) / 4;
                T.qbt4off.push_back(T.t4_doubles);
                T.t4fronts.push_back(f);
                T.t4dqo.push_back(T.dq4_ints);
                for (int g = 0; g < ngr; g++) {
                    T4Item it;
                    it.f = f; it.g = g; it.off = T.t4_doubles + (long long)g * qt4_doubles; it.dqo = T.dq4_ints;
                    T.t4items.push_back(it);
                }
                T.t4_doubles += (long long)ngr * qt4_doubles;
                T.dq4_ints += s.fn;
                xo += s.fm_ub; dqo += s.fn; wo += 2L * d.nslab * STM_NB;
                QbLevel &Q = T.qbig[l];
                Q.n++; Q.max_np = std::max(Q.max_np, s.npanels); Q.max_nslab = std::max(Q.max_nslab, d.nslab);
                Q.max_fm = std::max(Q.max_fm, s.fm_ub);
                Q.max_rsteps = std::max(Q.max_rsteps, (std::min(s.fp, s.fm_ub) + 31) / 32);
            } else {
                T.lds_qa[l] = std::max(T.lds_qa[l], need);
                T.lds_rs[l] = std::max(T.lds_rs[l], (int)std::min(stm_lds_rsolve(s.fp, s.fn), (long)INT_MAX));
            }
        }
        T.qbig[l].t4i_n = (int)T.t4items.size() - T.qbig[l].t4i_off;
        xf = std::max(xf, xo); dq = std::max(dq, dqo); wq = std::max(wq, wo);
        T.rtlc_ints = std::max(T.rtlc_ints, (long long)lco);
    }
    T.xf_doubles = xf; T.dq_ints = dq; T.wq_doubles = wq; T.wq4_doubles = 4 * wq;
    if (T.qb.empty()) T.qb.push_back(QbDesc());
    return T;
}

bool live_counts(LevelTables &T, const std::vector<FrontSym> &fs, const std::vector<FrontNum> &fnum, bool live, LiveCounts &L)
{
    bool changed = false;
    L.np.assign(T.qbig.size(), 0);
    L.rsteps.assign(T.qbig.size(), 0);
    L.rtsteps.assign(T.rtbig.size(), 0);
    for (size_t l = 0; l < T.qbig.size(); l++) {
        const QbLevel &Q = T.qbig[l];
        for (int q = 0; q < Q.n; q++) {
            QbDesc &d = T.qb[(size_t)(Q.off + q)];
            const FrontSym &s = fs[(size_t)d.f];
            const FrontNum &nm = fnum[(size_t)d.f];
            int npl = s.npanels;
            if (live) {
                const long lastcol = std::min((long)s.fn, (long)nm.fm + std::max(0L, (long)s.fp - (long)nm.rank));
                npl = (nm.fm <= 0) ? 0 : (int)std::min((long)s.npanels, (lastcol - 1) / STM_NB + 1);
            }
            if (d.np_live != npl) { d.np_live = npl; changed = true; }
            L.np[l] = std::max(L.np[l], npl);
            L.rsteps[l] = std::max(L.rsteps[l], live ? (int)((nm.rank + 31) / 32) : Q.max_rsteps);
        }
    }
    for (size_t l = 0; l < T.rtbig.size(); l++) {
        const RtLevel &R = T.rtbig[l];
        L.rtsteps[l] = live ? 0 : R.max_steps;
        for (int q = 0; q < R.n && live; q++) L.rtsteps[l] = std::max(L.rtsteps[l], (int)((fnum[(size_t)T.rtb[(size_t)(R.off + q)].f].rank + 31) / 32));
    }
    return changed;
}

void row_map(const std::vector<long> &Sleft, const std::vector<long> &Hip, const std::vector<int> &Hii, const std::vector<FrontSym> &fs,
             const std::vector<FrontNum> &fnum, long m, long n, std::vector<int> &Wmap, std::vector<int> &rowbase)
{
    const long nf = (long)fs.size();
    Wmap.assign((size_t)std::max(1L, m), 0);
    rowbase.assign((size_t)std::max(1L, nf), 0);
    long row1 = 0, row2 = m, run = 0;
    for (long i = Sleft[(size_t)n]; i < m; i++) Wmap[(size_t)i] = (int)--row2;
    for (long f = 0; f < nf; f++) {
        const int *Hi = Hii.data() + Hip[(size_t)f];
        const FrontNum &nm = fnum[(size_t)f];
        const long rm = nm.rank, fm = nm.fm;
        for (long i = 0; i < rm; i++) Wmap[(size_t)Hi[i]] = (int)row1++;
        const long cn = fs[(size_t)f].fn - fs[(size_t)f].fp;
        const long cm = std::min(fm - rm, cn);
        for (long i = fm - 1; i >= rm + cm; i--) Wmap[(size_t)Hi[i]] = (int)--row2;
        rowbase[(size_t)f] = (int)run;
        run += nm.rank;
    }
}

void rj_transpose(const std::vector<long> &Rj, long n, std::vector<int> &cp, std::vector<int> &slot)
{
    const size_t rjsize = Rj.size();
    cp.assign((size_t)n + 1, 0);
    slot.assign(std::max<size_t>(1, rjsize), 0);
    for (size_t p = 0; p < rjsize; p++) cp[(size_t)Rj[p] + 1]++;
    for (long j = 0; j < n; j++) cp[(size_t)j + 1] += cp[(size_t)j];
    std::vector<int> fill(cp.begin(), cp.end() - 1);
    for (size_t p = 0; p < rjsize; p++) slot[(size_t)fill[(size_t)Rj[p]]++] = (int)p;
}

void carried_view(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists, long ncol,
                  std::vector<FrontSym> &vs, std::vector<int> &blist, std::vector<int> &boff)
{
    blist.clear();
    boff.assign(LV.size() + 1, 0);
    for (size_t l = 0; l < LV.size(); l++) {
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = lists[(size_t)(LV[l].all_off + q)];
            const FrontSym &s = fs[(size_t)f];
            if ((long)s.col1 + s.fp > ncol) { blist.push_back(f); vs[(size_t)f].fp = (int)std::max(0L, ncol - (long)s.col1); }
        }
        boff[l + 1] = (int)blist.size();
    }
    if (blist.empty()) blist.push_back(0);
}

SelInvLayout selinv_layout(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists,
                           const std::vector<long> &Rj, long ncol)
{
    SelInvLayout Y;
    Y.sd.assign(std::max<size_t>(1, fs.size()), SiDesc());
    Y.lev_r.assign(LV.size(), 0);
    Y.lev_cn.assign(LV.size(), 0);
    for (size_t l = 0; l < LV.size(); l++) {
        long long w = 0;
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = lists[(size_t)(LV[l].all_off + q)];
            const FrontSym &s = fs[(size_t)f];
            SiDesc &d = Y.sd[(size_t)f];
            d.fp = (int)std::min<long>(s.fp, std::max(0L, ncol - (long)s.col1));
            d.check = d.fp == s.fp;
            d.cn = 0;
            if (d.check)
                while (s.fp + d.cn < s.fn && Rj[(size_t)(s.rp + s.fp + d.cn)] < ncol) d.cn++;
            d.rmax = std::min(d.fp, std::max(s.fm_ub, 0));
            const long long dim = (long long)d.rmax + d.cn;
            d.zoff = Y.zall; Y.zall += dim * dim;
            d.woff = w; w += (long long)std::max(d.rmax, 1) * dim;
            Y.lev_r[l] = std::max(Y.lev_r[l], d.rmax); Y.lev_cn[l] = std::max(Y.lev_cn[l], d.cn);
        }
        Y.wmax = std::max(Y.wmax, w);
    }
    return Y;
}

std::vector<int> column_fronts(const std::vector<long> &Super, long nf, long ncol)
{
    std::vector<int> cf((size_t)std::max(1L, ncol), 0);
    for (long f = 0; f < nf; f++)
        for (long k = Super[(size_t)f]; k < std::min<long>(Super[(size_t)f + 1], ncol); k++) cf[(size_t)k] = (int)f;
    return cf;
}

int resolve_pairs(const std::vector<FrontSym> &fs, const std::vector<long> &Super, const std::vector<long> &Rj, const long *Qfill, long ncol,
                  long npairs, const long *I, const long *J, std::vector<int> &trip, std::string &msg)
{
    std::vector<long> qinv((size_t)std::max(1L, ncol));          // caller's column -> R's order (Qfill maps [0, ncol) onto itself)
    for (long k = 0; k < ncol; k++) qinv[(size_t)(Qfill ? Qfill[k] : k)] = k;
    const std::vector<int> cf = column_fronts(Super, (long)fs.size(), ncol);
    trip.assign((size_t)(3 * npairs), 0);
    for (long p = 0; p < npairs; p++) {
        if (I[p] < 0 || I[p] >= ncol || J[p] < 0 || J[p] >= ncol) {
            msg = "covariance entries: pair " + std::to_string(p) + " = (" + std::to_string(I[p]) + ", " + std::to_string(J[p]) +
                  ") names a column outside 0 .. ncol - 1 = " + std::to_string(ncol - 1);
            return 1;
        }
        const long k1 = std::min(qinv[(size_t)I[p]], qinv[(size_t)J[p]]), k2 = std::max(qinv[(size_t)I[p]], qinv[(size_t)J[p]]);
        const int f = cf[(size_t)k1];
        const FrontSym &s = fs[(size_t)f];
        long l2 = k2 - s.col1;
        if (l2 >= s.fp) {
            const long *rj = Rj.data() + s.rp, *hit = std::lower_bound(rj + s.fp, rj + s.fn, k2);
            if (hit == rj + s.fn || *hit != k2) {
                msg = "covariance entries: pair " + std::to_string(p) + " = columns (" + std::to_string(I[p]) + ", " + std::to_string(J[p]) +
                      ") is outside the pattern of the selected inverse (the later column in R's order is no column of the front whose pivots hold the earlier one)";
                return 1;
            }
            l2 = hit - rj;
        }
        trip[(size_t)(3 * p)] = f; trip[(size_t)(3 * p + 1)] = (int)(k1 - s.col1); trip[(size_t)(3 * p + 2)] = (int)l2;
    }
    return 0;
}

void null_split(const std::vector<char> &rd, std::vector<int> &pc, std::vector<int> &jd)
{
    pc.clear(); jd.clear();
    for (size_t j = 0; j < rd.size(); j++) (rd[j] ? jd : pc).push_back((int)j);
}
NullSlabs null_slabs(long ncol, long want)
{
    long h = std::max(1L, want);
    while ((ncol + h - 1) / h > 65535) h *= 2;
    return {(int)h, (int)std::max(1L, (ncol + h - 1) / h)};
}
int null_panels(int d) { return (d + STM_NULL_NB - 1) / STM_NULL_NB; }
int null_panel_width(int d, int p) { return std::max(0, std::min(STM_NULL_NB, d - p * STM_NULL_NB)); }
long long null_lower_tiles(int d) { const long long t = null_panels(d); return t * (t + 1) / 2; }
}  // namespace restab
