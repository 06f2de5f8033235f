// la_table.cpp -- the LAv2 table (LAReference::GenerateApproximationData) and its C ABI.  The only unit that compiles LABuilder.
#include "inputs_state.hpp"

namespace {

constexpr uint32_t kLowBound = 64;   // LAReference.h:56
// periodDivisor: 2 for PerturbExtras::Disable, 8 for SimpleCompression (LAReference.cpp:12-19)
constexpr uint32_t kMaxLAStages = 1024;

template <class F> struct LABuilder {
    using Orb = typename orbit_of<F>::type;
    const LAParams p;
    const Orb &ob;
    LATable<F> &T;
    const int kPeriodDivisor;
    LABuilder(const Orb &o, LATable<F> &t) : p{}, ob(o), T(t), kPeriodDivisor(o.compressed ? 8 : 2) {}

    cplx_t<F> Z(uint64_t i) const { return hc_from_hr(ob.x[i], ob.y[i]); } // GetComplex<SubType>()

    uint32_t la_size() const { return (uint32_t)T.las.size(); }

    // Shared prologue of CreateLAFromOrbit / CreateLAFromOrbitMT (LAReference.cpp:40-151 == :256-352).
    // Returns 0 = finished with `false`, 1 = continue into the main scan.
    int stage0_prologue(uint32_t maxRef, LAInfo<F> &LA, uint32_t &i, uint32_t &Period, uint32_t &PeriodBegin,
                        uint32_t &PeriodEnd, uint32_t &nextStageLAIndex)
    {
        T.isValid = false;
        T.stages.assign(kMaxLAStages, fs_la_stage_u32{0, 0});
        T.useAT = false;
        T.stageCount = 0;
        T.stages[0].LAIndex = 0;

        Period = 0;
        LA = la_init<F>(p, mk<F>::czero());
        LA = la_step_new(p, LA, Z(1));
        nextStageLAIndex = 0;
        if (LA.ZCoeff.re == scalar_t<F>(0) && LA.ZCoeff.im == scalar_t<F>(0)) // isZCoeffZero
            return 0;

        for (i = 2; i < maxRef; i++) {
            LAInfo<F> NewLA;
            const bool PeriodDetected = la_step(p, LA, NewLA, Z(i));
            if (!PeriodDetected) {
                LA = NewLA;
                continue;
            }
            Period = i;
            LA.StepLength = Period;
            LA.NextStageLAIndex = nextStageLAIndex;
            T.las.push_back(LA);
            nextStageLAIndex = i;
            if (i + 1 < maxRef) {
                LA = la_step_new(p, la_init<F>(p, Z(i)), Z(i + 1));
                i += 2;
            } else {
                LA = la_init<F>(p, Z(i));
                i += 1;
            }
            break;
        }
        T.stageCount = 1;
        PeriodBegin = Period;
        PeriodEnd = PeriodBegin + Period;

        if (Period == 0) {
            if (maxRef > kLowBound) {
                LA = la_step_new(p, la_init<F>(p, Z(0)), Z(1));
                nextStageLAIndex = 0;
                i = 2;
                const double NthRoot = std::round(std::log2((double)maxRef) / kPeriodDivisor);
                Period = (uint32_t)std::round(std::pow((double)maxRef, 1.0 / NthRoot));
                PeriodBegin = 0;
                PeriodEnd = Period;
            } else {
                LA.StepLength = maxRef;
                LA.NextStageLAIndex = nextStageLAIndex;
                T.las.push_back(LA);
                T.las.push_back(la_init<F>(p, Z(maxRef)));
                T.stages[0].MacroItCount = 1;
                return 0;
            }
        } else if (Period > kLowBound) {
            T.las.pop_back();
            LA = la_step_new(p, la_init<F>(p, Z(0)), Z(1));
            nextStageLAIndex = 0;
            i = 2;
            const double NthRoot = std::round(std::log2((double)maxRef) / kPeriodDivisor);
            Period = (uint32_t)std::round(std::pow((double)maxRef, 1.0 / NthRoot));
            PeriodBegin = 0;
            PeriodEnd = Period;
        }
        return 1;
    }

    // CreateLAFromOrbit, LAReference.cpp:28-210
    bool create_stage0_st(uint32_t maxRef)
    {
        LAInfo<F> LA;
        uint32_t i, Period, PeriodBegin, PeriodEnd, nextIdx;
        if (!stage0_prologue(maxRef, LA, i, Period, PeriodBegin, PeriodEnd, nextIdx))
            return false;
        for (; i < maxRef; i++) {
            LAInfo<F> NewLA;
            const bool PeriodDetected = la_step(p, LA, NewLA, Z(i));
            if (!PeriodDetected && i < PeriodEnd) {
                LA = NewLA;
                continue;
            }
            LA.StepLength = i - PeriodBegin;
            LA.NextStageLAIndex = nextIdx;
            T.las.push_back(LA);
            nextIdx = i;
            PeriodBegin = i;
            PeriodEnd = PeriodBegin + Period;
            const uint32_t ip1 = i + 1;
            const bool detected = la_detect_period(p, NewLA, Z(ip1));
            if (detected || ip1 >= maxRef) {
                LA = la_init<F>(p, Z(i));
            } else {
                LA = la_step_new(p, la_init<F>(p, Z(i)), Z(ip1));
                i++;
            }
        }
        LA.StepLength = i - PeriodBegin;
        LA.NextStageLAIndex = nextIdx;
        T.las.push_back(LA);
        T.stages[0].MacroItCount = la_size();
        LAInfo<F> LA2 = la_init<F>(p, Z(maxRef));
        T.las.push_back(LA2);
        return true;
    }

    // CreateNewLAStage, LAReference.cpp:774-966
    bool create_new_stage(uint32_t maxRef)
    {
        LAInfo<F> LA;
        uint32_t liStep = 0, liNext = 0; // LAI
        uint32_t i, PeriodBegin, PeriodEnd;
        const uint32_t PrevStage = T.stageCount - 1;
        const uint32_t CurrentStage = T.stageCount;
        const uint32_t PrevStageLAIndex = T.stages[PrevStage].LAIndex;
        const uint32_t PrevStageMacroItCount = T.stages[PrevStage].MacroItCount;
        const LAInfo<F> PrevStageLA = T.las[PrevStageLAIndex];
        const uint32_t PrevStageLAI_Step = PrevStageLA.StepLength;
        const LAInfo<F> PrevStageLAp1 = T.las[PrevStageLAIndex + 1];
        const uint32_t PrevStageLAIp1_Step = PrevStageLAp1.StepLength;
        uint32_t Period = 0;

        if (CurrentStage >= kMaxLAStages)
            return false;
        T.stages[CurrentStage].LAIndex = la_size();

        LA = la_composite_new(p, PrevStageLA, PrevStageLAp1);
        liNext = 0;
        i = PrevStageLAI_Step + PrevStageLAIp1_Step;
        uint32_t j;
        for (j = 2; j < PrevStageMacroItCount; j++) {
            LAInfo<F> NewLA;
            const uint32_t idxj = PrevStageLAIndex + j;
            const LAInfo<F> PrevStageLAj = T.las[idxj];
            const bool PeriodDetected = la_composite(p, LA, NewLA, PrevStageLAj);
            if (PeriodDetected) {
                if (PrevStageLAj.LAThreshold.m == scalar_t<F>(0)) // isLAThresholdZero
                    break;
                Period = i;
                liStep = Period;
                LA.StepLength = liStep;
                LA.NextStageLAIndex = liNext;
                T.las.push_back(LA);
                liNext = j;
                const LAInfo<F> PrevStageLAjp1 = T.las[idxj + 1];
                if (la_detect_period(p, NewLA, PrevStageLAjp1.Ref) || j + 1 >= PrevStageMacroItCount) {
                    LA = PrevStageLAj;
                    i += PrevStageLAj.StepLength;
                    j++;
                } else {
                    LA = la_composite_new(p, PrevStageLAj, PrevStageLAjp1);
                    i += PrevStageLAj.StepLength + PrevStageLAjp1.StepLength;
                    j += 2;
                }
                break;
            }
            LA = NewLA;
            i += T.las[PrevStageLAIndex + j].StepLength;
        }
        T.stageCount++;

        PeriodBegin = Period;
        PeriodEnd = PeriodBegin + Period;

        if (Period == 0) {
            if (maxRef > PrevStageLAI_Step * kLowBound) {
                LA = la_composite_new(p, PrevStageLA, PrevStageLAp1);
                i = PrevStageLAI_Step + PrevStageLAIp1_Step;
                liNext = 0;
                j = 2;
                const double Ratio = ((double)maxRef) / PrevStageLAI_Step;
                const double NthRoot = std::round(std::log2((double)maxRef) / kPeriodDivisor);
                Period = PrevStageLAI_Step * (uint32_t)std::round(std::pow(Ratio, 1.0 / NthRoot));
                PeriodBegin = 0;
                PeriodEnd = Period;
            } else {
                liStep = maxRef;
                LA.StepLength = liStep;
                LA.NextStageLAIndex = liNext;
                T.las.push_back(LA);
                LAInfo<F> LA2 = la_init<F>(p, Z(maxRef));
                T.las.push_back(LA2);
                T.stages[CurrentStage].MacroItCount = 1;
                return false;
            }
        } else if (Period > PrevStageLAI_Step * kLowBound) {
            T.las.pop_back();
            LA = la_composite_new(p, PrevStageLA, PrevStageLAp1);
            i = PrevStageLAI_Step + PrevStageLAIp1_Step;
            liNext = 0;
            j = 2;
            const double Ratio = ((double)Period) / PrevStageLAI_Step;
            const double NthRoot = std::round(std::log2((double)maxRef) / kPeriodDivisor);
            Period = PrevStageLAI_Step * ((uint32_t)std::round(std::pow(Ratio, 1.0 / NthRoot)));
            PeriodBegin = 0;
            PeriodEnd = Period;
        }

        for (; j < PrevStageMacroItCount; j++) {
            LAInfo<F> NewLA;
            const uint32_t idxj = PrevStageLAIndex + j;
            const LAInfo<F> PrevStageLAj = T.las[idxj];
            const bool PeriodDetected = la_composite(p, LA, NewLA, PrevStageLAj);
            if (PeriodDetected || i >= PeriodEnd) {
                liStep = i - PeriodBegin;
                LA.StepLength = liStep;
                LA.NextStageLAIndex = liNext;
                T.las.push_back(LA);
                liNext = j;
                PeriodBegin = i;
                PeriodEnd = PeriodBegin + Period;
                const LAInfo<F> PrevStageLAjp1 = T.las[idxj + 1];
                if (la_detect_period(p, NewLA, PrevStageLAjp1.Ref) || j + 1 >= PrevStageMacroItCount) {
                    LA = PrevStageLAj;
                } else {
                    LA = la_composite_new(p, PrevStageLAj, PrevStageLAjp1);
                    i += T.las[idxj].StepLength;
                    j++;
                }
            } else {
                LA = NewLA;
            }
            i += T.las[PrevStageLAIndex + j].StepLength;
        }
        liStep = i - PeriodBegin;
        LA.StepLength = liStep;
        LA.NextStageLAIndex = liNext;
        T.las.push_back(LA);
        T.stages[CurrentStage].MacroItCount = la_size() - T.stages[CurrentStage].LAIndex;
        LA = la_init<F>(p, Z(maxRef));
        T.las.push_back(LA);
        return true;
    }

    // CreateATFromLA, LAReference.cpp:1050-1074
    // UseSmallExponents = UsingDblflt (RefOrbitCalc.cpp:2346): true when the HDRFloat<double> table is built to be
    // converted to 2x32, so that the AT escape radius fits a binary32 mantissa (lim = 2^32 instead of 2^256).
    bool useSmallExponents = false;
    void create_at(real_t<F> radius, bool useSmallExponents)
    {
        const real_t<F> SqrRadius = hr_reduced(hr_square(radius));
        for (uint32_t Stage = T.stageCount; Stage > 0;) {
            Stage--;
            const uint32_t LAIndex = T.stages[Stage].LAIndex;
            la_create_at(T.las[LAIndex], T.at, T.las[LAIndex + 1], useSmallExponents);
            T.at.StepLength = T.las[LAIndex].StepLength;
            if (T.at.StepLength > 0 && at_usable(T.at, SqrRadius)) {
                T.useAT = true;
                return;
            }
        }
        T.useAT = false;
    }

    // GenerateApproximationData, LAReference.cpp:971-1013
    void generate(int threads)
    {
        T.las.clear();
        const uint32_t maxRef = (uint32_t)ob.x.size() - 1;
        if (maxRef == 0) {
            T.isValid = false;
            return;
        }
        bool PeriodDetected;
        // CreateLAFromOrbitMT falls back to the single-threaded scan when
        // maxRefIteration / 50000 (capped by hardware_concurrency) is < 2 (LAReference.cpp:236-251).
        size_t threadCount = maxRef / 50000;
        if (threadCount > (size_t)threads)
            threadCount = threads;
        if (threadCount <= 1) {
            PeriodDetected = create_stage0_st(maxRef);
        } else {
            PeriodDetected = create_stage0_mt(maxRef, threadCount);
        }
        if (!PeriodDetected)
            return;
        while (create_new_stage(maxRef)) {
        }
        create_at(ob.maxRadius, useSmallExponents);
        T.isValid = true;
    }

    bool create_stage0_mt(uint32_t maxRef, size_t threadCount);
};

// CreateLAFromOrbitMT, LAReference.cpp:215-770, replayed sequentially.  The reference runs a "Starter"
// (thread 0, continues the scan from the prologue) and Workers 1..N-1 that each begin at a fixed orbit
// index, find their first period boundary, publish it (StartIndexPromise) and scan on until they pass
// the *next* worker's published start.  All cross-thread values are futures, so the outcome does not
// depend on timing: replaying the workers from last to first and the starter last reproduces it.
template <class F> bool LABuilder<F>::create_stage0_mt(uint32_t maxRef, size_t ThreadCount)
{
    LAInfo<F> LA;
    uint32_t i, Period, PeriodBegin, PeriodEnd, nextIdx;
    if (!stage0_prologue(maxRef, LA, i, Period, PeriodBegin, PeriodEnd, nextIdx))
        return false;

    std::vector<int64_t> StartIndex(ThreadCount, 0);
    std::vector<int64_t> FinishIndex(ThreadCount, 0);
    std::vector<std::vector<LAInfo<F>>> LAsPerThread(ThreadCount);
    std::vector<LAInfo<F>> LastLAPerThread(ThreadCount);

    // Workers, last first (each only waits on StartIndexFuture of higher thread ids).
    for (size_t ThreadID = ThreadCount - 1; ThreadID >= 1; ThreadID--) {
        size_t NextThread = ThreadID + 1;
        const size_t LastThread = ThreadCount - 1;
        const uint32_t Begin = (uint32_t)((uint64_t)maxRef * ThreadID / ThreadCount);
        uint32_t j = Begin;
        const uint32_t End = (uint32_t)((uint64_t)maxRef * NextThread / ThreadCount);

        uint32_t liNext = j;
        LAInfo<F> LA_2 = la_step_new(p, la_init<F>(p, Z(j)), Z(j + 1));
        uint32_t j2 = j + 2;
        LAInfo<F> LA_ = la_step_new(p, la_init<F>(p, Z(j - 1)), Z(j));
        uint32_t j1 = j + 1;

        uint32_t wPeriodBegin = 0, wPeriodEnd = 0;
        bool PeriodDetected = false, PeriodDetected2 = false;

        for (; j2 < maxRef || j1 < maxRef; j1++, j2++) {
            LAInfo<F> NewLA;
            PeriodDetected = la_step(p, LA_, NewLA, Z(j1));
            if (PeriodDetected) {
                liNext = j1;
                wPeriodBegin = j1;
                wPeriodEnd = wPeriodBegin + Period;
                if (j1 + 1 >= maxRef) {
                    LA_ = la_init<F>(p, Z(j1));
                    j1 += 1;
                } else {
                    LA_ = la_step_new(p, la_init<F>(p, Z(j1)), Z(j1 + 1));
                    j1 += 2;
                }
                break;
            }
            LA_ = NewLA;
            if (j2 < maxRef) {
                LAInfo<F> NewLA2;
                PeriodDetected2 = la_step(p, LA_2, NewLA2, Z(j2));
                if (PeriodDetected2) {
                    liNext = j2;
                    wPeriodBegin = j2;
                    wPeriodEnd = wPeriodBegin + Period;
                    const uint32_t jp1 = j2 + 1;
                    if (jp1 >= maxRef) {
                        LA_2 = la_init<F>(p, Z(j2));
                        j2++;
                    } else {
                        LA_2 = la_step_new(p, la_init<F>(p, Z(j2)), Z(jp1));
                        j2 += 2;
                    }
                    break;
                }
                LA_2 = NewLA2;
            }
        }
        if (PeriodDetected2) {
            LA_ = LA_2;
            j = j2;
        } else if (PeriodDetected) {
            j = j1;
        } else {
            j = maxRef;
        }

        if (ThreadID == LastThread || (j >= Begin && j < End)) {
            StartIndex[ThreadID] = j;
        } else {
            const int64_t nextStart = StartIndex[NextThread];
            StartIndex[ThreadID] = nextStart;
            FinishIndex[ThreadID] = -1;
            continue;
        }

        bool returned = false;
        for (; j < maxRef; j++) {
            LAInfo<F> NewLA;
            PeriodDetected = la_step(p, LA_, NewLA, Z(j));
            if (!PeriodDetected && j < wPeriodEnd) {
                LA_ = NewLA;
                continue;
            }
            LA_.StepLength = j - wPeriodBegin;
            LA_.NextStageLAIndex = liNext;
            LAsPerThread[ThreadID].push_back(LA_);
            liNext = j;
            wPeriodBegin = j;
            wPeriodEnd = wPeriodBegin + Period;
            const uint32_t jp1 = j + 1;
            const bool detected = la_detect_period(p, NewLA, Z(jp1));
            if (detected || jp1 >= maxRef) {
                LA_ = la_init<F>(p, Z(j));
            } else {
                LA_ = la_step_new(p, la_init<F>(p, Z(j)), Z(jp1));
                j++;
            }
            if (j > End) {
                if (j >= maxRef)
                    break;
                if (NextThread < ThreadCount) {
                    const int64_t nextStart = StartIndex[NextThread];
                    if (nextStart < 0) {
                        returned = true;
                        break;
                    }
                    if ((int64_t)j == nextStart - 1) {
                        j++;
                        break;
                    } else if ((int64_t)j >= nextStart) {
                        NextThread++;
                    }
                }
            }
        }
        if (returned)
            continue;
        FinishIndex[ThreadID] = (int64_t)j;
        LA_.StepLength = j - wPeriodBegin;
        LA_.NextStageLAIndex = liNext;
        LastLAPerThread[ThreadID] = LA_;
    }

    // Starter (thread 0), LAReference.cpp:392-484.
    {
        const uint32_t threadBoundary = maxRef / (uint32_t)ThreadCount;
        size_t NextThread = 1;
        bool returned = false;
        for (; i < maxRef; i++) {
            LAInfo<F> NewLA;
            const bool PeriodDetected = la_step(p, LA, NewLA, Z(i));
            if (!PeriodDetected && i < PeriodEnd) {
                LA = NewLA;
                continue;
            }
            LA.StepLength = i - PeriodBegin;
            LA.NextStageLAIndex = nextIdx;
            T.las.push_back(LA);
            nextIdx = i;
            PeriodBegin = i;
            PeriodEnd = PeriodBegin + Period;
            const uint32_t ip1 = i + 1;
            const bool detected = la_detect_period(p, NewLA, Z(ip1));
            if (detected || ip1 >= maxRef) {
                LA = la_init<F>(p, Z(i));
            } else {
                LA = la_step_new(p, la_init<F>(p, Z(i)), Z(ip1));
                i++;
            }
            if (i > threadBoundary) {
                if (i >= maxRef)
                    break;
                if (NextThread < ThreadCount) {
                    const int64_t nextStart = StartIndex[NextThread];
                    if (nextStart < 0) {
                        returned = true;
                        break;
                    }
                    if ((int64_t)i == nextStart - 1) {
                        i++;
                        break;
                    } else if ((int64_t)i >= nextStart) {
                        NextThread++;
                    }
                }
            }
        }
        if (!returned) {
            FinishIndex[0] = (int64_t)i;
            LA.StepLength = i - PeriodBegin;
            LA.NextStageLAIndex = nextIdx;
            LastLAPerThread[0] = LA;
        }
    }

    // Stitch, LAReference.cpp:711-760.
    {
        size_t lastThreadToAdd = 0;
        size_t index = 0;
        size_t j = index;
        while ((index < ThreadCount - 1) && (FinishIndex[j] > StartIndex[index + 1]))
            index++;
        index++;
        for (; index < ThreadCount; index++) {
            const auto &threadData = LAsPerThread[index];
            T.las.insert(T.las.end(), threadData.begin(), threadData.end());
            if (FinishIndex[index] > StartIndex[index])
                lastThreadToAdd = index;
            j = index;
            while ((index < ThreadCount - 1) && (FinishIndex[j] > StartIndex[index + 1]))
                index++;
        }
        T.las.push_back(LastLAPerThread[lastThreadToAdd]);
    }
    T.stages[0].MacroItCount = la_size();
    T.las.push_back(la_init<F>(p, Z(maxRef)));
    return true;
}

} // namespace

template <class F> void la_generate(const typename orbit_of<F>::type &ob, LATable<F> &t, int host_threads, bool use_small_exponents)
{
    LABuilder<F> b(ob, t);
    b.useSmallExponents = use_small_exponents;
    b.generate(host_threads);
    t.packedStages.assign(t.stages.begin(), t.stages.begin() + std::min<size_t>(t.stages.size(), t.stageCount));
}
template void la_generate<float>(const OrbitT<float> &, LATable<float> &, int, bool);
template void la_generate<double>(const OrbitT<double> &, LATable<double> &, int, bool);
template void la_generate<plain<float>>(const PlainOrbit<float> &, LATable<plain<float>> &, int, bool);
template void la_generate<plain<double>>(const PlainOrbit<double> &, LATable<plain<double>> &, int, bool);

namespace {
template <class F> void pack_la(const LATable<F> &t, std::vector<fs_la_hdr32_u32> *o32, std::vector<fs_la_hdr64_u32> *o64)
{
    for (size_t k = 0; k < t.las.size(); k++) {
        const auto &s = t.las[k];
        if (o32) {
            fs_la_hdr32_u32 r;
            r.Ref = fs_cplx_hdr32{(float)s.Ref.re, (float)s.Ref.im, s.Ref.e};
            r.ZCoeff = fs_cplx_hdr32{(float)s.ZCoeff.re, (float)s.ZCoeff.im, s.ZCoeff.e};
            r.CCoeff = fs_cplx_hdr32{(float)s.CCoeff.re, (float)s.CCoeff.im, s.CCoeff.e};
            r.LAThreshold = fs_real_hdr32{(float)s.LAThreshold.m, s.LAThreshold.e};
            r.LAThresholdC = fs_real_hdr32{(float)s.LAThresholdC.m, s.LAThresholdC.e};
            r.MinMag = fs_real_hdr32{(float)s.MinMag.m, s.MinMag.e};
            r.StepLength = s.StepLength;
            r.NextStageLAIndex = s.NextStageLAIndex;
            o32->push_back(r);
        } else {
            fs_la_hdr64_u32 r;
            memset(&r, 0, sizeof(r));
            r.Ref = fs_cplx_hdr64{(double)s.Ref.re, (double)s.Ref.im, s.Ref.e, 0};
            r.ZCoeff = fs_cplx_hdr64{(double)s.ZCoeff.re, (double)s.ZCoeff.im, s.ZCoeff.e, 0};
            r.CCoeff = fs_cplx_hdr64{(double)s.CCoeff.re, (double)s.CCoeff.im, s.CCoeff.e, 0};
            r.LAThreshold = fs_real_hdr64{(double)s.LAThreshold.m, s.LAThreshold.e, 0};
            r.LAThresholdC = fs_real_hdr64{(double)s.LAThresholdC.m, s.LAThresholdC.e, 0};
            r.MinMag = fs_real_hdr64{(double)s.MinMag.m, s.MinMag.e, 0};
            r.StepLength = s.StepLength;
            r.NextStageLAIndex = s.NextStageLAIndex;
            o64->push_back(r);
        }
    }
}
} // namespace

// The LAParameters every table in this file is built with (la_math.hpp LAParams = the reference's defaults,
// LAParameters.h:66-75): {detectionMethod, LAThresholdScaleExp, LAThresholdCScaleExp, Stage0PeriodDetectionThreshold2Exp,
// PeriodDetectionThreshold2Exp, Stage0PeriodDetectionThresholdExp, PeriodDetectionThresholdExp}.
extern "C" void fsh_la_default_params(int32_t out[7])
{
    const LAParams p{};
    out[0] = p.detectionMethod, out[1] = p.laThresholdScaleExp, out[2] = p.laThresholdCScaleExp;
    out[3] = p.stage0PeriodDetectionThreshold2Exp, out[4] = p.periodDetectionThreshold2Exp;
    out[5] = p.stage0PeriodDetectionThresholdExp, out[6] = p.periodDetectionThresholdExp;
}

extern "C" fsh_la *fsh_la_create_ex(const fsh_orbit *o, int host_threads, int use_small_exponents);
extern "C" fsh_la *fsh_la_create(const fsh_orbit *o, int host_threads) { return fsh_la_create_ex(o, host_threads, 0); }
extern "C" fsh_la *fsh_la_create_ex(const fsh_orbit *o, int host_threads, int use_small_exponents)
{
    auto la = std::make_unique<fsh_la>();
    la->is64 = o->is64;
    const int th = host_threads < 1 ? 1 : host_threads;
    if (o->is64) {
        la_generate<double>(o->d, la->t64, th, use_small_exponents != 0);
        pack_la<double>(la->t64, nullptr, &la->packed64);
    } else {
        la_generate<float>(o->f, la->t32, th);
        pack_la<float>(la->t32, &la->t32.packed32, nullptr);
    }
    return la.release();
}
extern "C" fsh_la *fsh_la_create_hdr32(const fsh_orbit *o, int host_threads)
{
    return o->is64 ? nullptr : fsh_la_create(o, host_threads);
}
extern "C" void fsh_la_destroy(fsh_la *l) { delete l; }
extern "C" int fsh_la_is64(const fsh_la *l) { return l->is64; }
extern "C" uint32_t fsh_la_count(const fsh_la *l)
{
    return l->is64 ? (uint32_t)l->packed64.size() : (uint32_t)l->t32.packed32.size();
}
extern "C" const void *fsh_la_data(const fsh_la *l)
{
    return l->is64 ? (const void *)l->packed64.data() : (const void *)l->t32.packed32.data();
}
extern "C" uint32_t fsh_la_stage_count(const fsh_la *l) { return l->is64 ? l->t64.stageCount : l->t32.stageCount; }
extern "C" const fs_la_stage_u32 *fsh_la_stages(const fsh_la *l)
{
    return l->is64 ? l->t64.packedStages.data() : l->t32.packedStages.data();
}
extern "C" int fsh_la_is_valid(const fsh_la *l) { return (l->is64 ? l->t64.isValid : l->t32.isValid) ? 1 : 0; }
extern "C" int fsh_la_use_at(const fsh_la *l) { return (l->is64 ? l->t64.useAT : l->t32.useAT) ? 1 : 0; }
// out: fs_at_hdr32_u32 (116 B) or fs_at_hdr64_u32 (232 B) depending on fsh_la_is64().
extern "C" void fsh_la_at(const fsh_la *l, void *outp)
{
    if (!l->is64) {
        const auto &a = l->t32.at;
        fs_at_hdr32_u32 *out = (fs_at_hdr32_u32 *)outp;
        auto R = [](hreal<float> h) { return fs_real_hdr32{h.m, h.e}; };
        auto C = [](hcplx<float> c) { return fs_cplx_hdr32{c.re, c.im, c.e}; };
        out->StepLength = a.StepLength;
        out->ThresholdC = R(a.ThresholdC);
        out->SqrEscapeRadius = R(a.SqrEscapeRadius);
        out->RefC = C(a.RefC);
        out->ZCoeff = C(a.ZCoeff);
        out->CCoeff = C(a.CCoeff);
        out->InvZCoeff = C(a.InvZCoeff);
        out->CCoeffSqrInvZCoeff = C(a.CCoeffSqrInvZCoeff);
        out->CCoeffInvZCoeff = C(a.CCoeffInvZCoeff);
        out->CCoeffNormSqr = R(a.CCoeffNormSqr);
        out->RefCNormSqr = R(a.RefCNormSqr);
        out->factor = R(a.factor);
    } else {
        const auto &a = l->t64.at;
        fs_at_hdr64_u32 *out = (fs_at_hdr64_u32 *)outp;
        memset(out, 0, sizeof(*out));
        auto R = [](hreal<double> h) { return fs_real_hdr64{h.m, h.e, 0}; };
        auto C = [](hcplx<double> c) { return fs_cplx_hdr64{c.re, c.im, c.e, 0}; };
        out->StepLength = a.StepLength;
        out->ThresholdC = R(a.ThresholdC);
        out->SqrEscapeRadius = R(a.SqrEscapeRadius);
        out->RefC = C(a.RefC);
        out->ZCoeff = C(a.ZCoeff);
        out->CCoeff = C(a.CCoeff);
        out->InvZCoeff = C(a.InvZCoeff);
        out->CCoeffSqrInvZCoeff = C(a.CCoeffSqrInvZCoeff);
        out->CCoeffInvZCoeff = C(a.CCoeffInvZCoeff);
        out->CCoeffNormSqr = R(a.CCoeffNormSqr);
        out->RefCNormSqr = R(a.RefCNormSqr);
        out->factor = R(a.factor);
    }
}
