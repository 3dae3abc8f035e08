// duet_tune_derive.hip.h -- what the T1-T5 tree of predict_hp (src/duet/sv_phasing_fn.py:112-139) compares, from one feature
// record: shared by the sweep (duet_tune.hip: decide_vec) and the line of one axis (duet_tune_line.hip), so that a threshold
// taken from a candidate's feature compares equal to it.  Included inside each unit's anonymous namespace.
#ifndef DUET_TUNE_DERIVE_HIP_H
#define DUET_TUNE_DERIVE_HIP_H

// What the tree compares, in binary64 exactly as Python computes it (:112-139)
struct Derived {
    double sv_ratio, hr, diff, totsc, svread, refread, hap0;
    uint32_t cls;
    bool onehap, a1pos, t1gt;
};

__device__ __forceinline__ Derived derive(const duet_tune_feature &f)
{
    Derived d;
    d.cls = f.cls;
    d.hr = (double)f.allhap / (double)f.deg;                                        // :112
    const double a1 = f.hap1 > 0 ? (double)f.t1 / (double)f.hap1 : 0.0;             // :113-114
    const double a2 = f.hap2 > 0 ? (double)f.t2 / (double)f.hap2 : 0.0;             // :115-116
    d.sv_ratio = (double)f.svread / (double)((uint64_t)f.svread + (uint64_t)f.refread);   // :123
    const uint64_t lo = f.t1 < f.t2 ? f.t1 : f.t2, hi = f.t1 < f.t2 ? f.t2 : f.t1;
    d.totsc = lo > 0 ? (double)hi / (double)lo : 0.0;                               // :124-125
    d.onehap = lo == 0 && hi != 0;                                                  // onehap_totsc != 0, :126-127
    d.diff = fabs(a2 - a1);                                                         // :132
    d.svread = (double)f.svread;
    d.refread = (double)f.refread;
    d.hap0 = (double)f.hap0;
    d.a1pos = a1 > 0;
    d.t1gt = f.t1 > f.t2;
    return d;
}

#endif
