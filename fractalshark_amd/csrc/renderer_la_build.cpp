#include "renderer_state.hpp"

#include <cmath>

#include "la_math.hpp"

using namespace fsr;

// ---- LAv2 table built on the device (kernels_la.hip): the scalar decisions of LAReference.cpp on the host, everything
// that touches the orbit or a record on the device.  See the header of kernels_la.hip for the algorithm.
namespace {

// Work memory that outlives a call: grown, never shrunk, handed out from the start on every use.
hipError_t arena_reserve(fs_renderer *r, size_t bytes)
{
    if (r->arena.cap >= bytes)
        return hipSuccess;
    return buf_reserve(r, r->arena, bytes + bytes / 4, kInput); // some slack: the next orbit of a zoom sequence is usually a little longer
}

// Work arrays of one fs_build_la call, carved out of the renderer's arena (no allocation once the arena has grown to the
// largest orbit seen): 256-byte aligned slices handed out front to back.
struct ArenaSlice {
    void *p;
    template <class T> T *as() const { return (T *)p; }
};
struct ArenaCarver {
    char *base;
    size_t used = 0;
    explicit ArenaCarver(void *b) : base((char *)b) {}
    static size_t padded(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }
    template <class T> T *take(size_t bytes)
    {
        T *p = (T *)(base + used);
        used += padded(bytes ? bytes : 16);
        return p;
    }
};

template <class F> void pack_at(const fs::la::ATInfoT<F> &a, fs_renderer *r);
template <> void pack_at<float>(const fs::la::ATInfoT<float> &a, fs_renderer *r)
{
    auto R = [](fs::hreal<float> h) { return fs_real_hdr32{h.m, h.e}; };
    auto C = [](fs::hcplx<float> c) { return fs_cplx_hdr32{c.re, c.im, c.e}; };
    fs_at_hdr32_u32 &o = r->at;
    memset(&o, 0, sizeof(o));
    o.StepLength = a.StepLength;
    o.ThresholdC = R(a.ThresholdC), o.SqrEscapeRadius = R(a.SqrEscapeRadius);
    o.RefC = C(a.RefC), o.ZCoeff = C(a.ZCoeff), o.CCoeff = C(a.CCoeff), o.InvZCoeff = C(a.InvZCoeff);
    o.CCoeffSqrInvZCoeff = C(a.CCoeffSqrInvZCoeff), o.CCoeffInvZCoeff = C(a.CCoeffInvZCoeff);
    o.CCoeffNormSqr = R(a.CCoeffNormSqr), o.RefCNormSqr = R(a.RefCNormSqr), o.factor = R(a.factor);
}
template <> void pack_at<double>(const fs::la::ATInfoT<double> &a, fs_renderer *r)
{
    auto R = [](fs::hreal<double> h) { return fs_real_hdr64{h.m, h.e, 0}; };
    auto C = [](fs::hcplx<double> c) { return fs_cplx_hdr64{c.re, c.im, c.e, 0}; };
    fs_at_hdr64_u32 &o = r->at64;
    memset(&o, 0, sizeof(o));
    o.StepLength = a.StepLength;
    o.ThresholdC = R(a.ThresholdC), o.SqrEscapeRadius = R(a.SqrEscapeRadius);
    o.RefC = C(a.RefC), o.ZCoeff = C(a.ZCoeff), o.CCoeff = C(a.CCoeff), o.InvZCoeff = C(a.InvZCoeff);
    o.CCoeffSqrInvZCoeff = C(a.CCoeffSqrInvZCoeff), o.CCoeffInvZCoeff = C(a.CCoeffInvZCoeff);
    o.CCoeffNormSqr = R(a.CCoeffNormSqr), o.RefCNormSqr = R(a.RefCNormSqr), o.factor = R(a.factor);
}

constexpr uint32_t kLaLowBound = 64;    // LAReference.h:56
constexpr uint32_t kLaMaxStages = 1024; // LAReference.h
constexpr uint32_t kLaTerm = 0xFFFFFFFFu;

template <class F> uint32_t build_la(fs_renderer *r, const void *max_radius, int use_small_exponents, int host_threads)
{
    using Rec = fs::la::LAInfo<F>;
    using HR = fs::hreal<F>;
    hipStream_t s = r->compute;
    const void *zref = sizeof(F) == 4 ? (const void *)r->zref : (const void *)r->zref64;
    // state numbers (2 per element) and record indices are 32-bit on the device: an orbit of 2^31 entries does not fit
    // (its prepared form alone would be 32 GiB of float4); refuse instead of truncating
    if (r->orbit_uncompressed >= (1ull << 31))
        return FS_ERR_UNSUPPORTED;
    const uint32_t maxRef = (uint32_t)r->orbit_uncompressed - 1u; // entries 0 .. maxRef
    const int periodDivisor = r->orbit_size != r->orbit_uncompressed ? 8 : 2; // LAReference.cpp:12-19
    if (r->orbit_uncompressed < 3)
        return FS_ERR_UNSUPPORTED; // (maxRefIteration == 0: no table, LAReference.cpp:981-984; one step: left to the host builder)
    // capacity: a stage never holds more records than elements it was folded from (+ its tail record)
    const size_t cap_states = 2u * ((size_t)maxRef + 2u);
    // all stages: stage k+1 holds at most half of stage k (+2), so 2 * maxRef + slack bounds the sum
    const size_t cap_recs = 2u * (size_t)maxRef + 64u * kLaLowBound;
    const size_t sizes[13] = {sizeof(HR) * (maxRef + 2u), sizeof(HR) * (maxRef + 2u), 4u * (maxRef + 2u), 4u * (maxRef + 3u),
                              4u * cap_states,            4u * cap_states,            4u * cap_states,     4u * cap_states,
                              4u * (cap_states + 1u),     sizeof(Rec) * cap_recs,     64,                  4u * kLaMaxStages,
                              sizeof(fs::la::ATInfoT<F>)};
    size_t total = 0;
    for (size_t b : sizes)
        total += ArenaCarver::padded(b);
    FS_TRY(arena_reserve(r, total));
    ArenaCarver carve(r->arena.p);
    ArenaSlice chebv{carve.take<char>(sizes[0])}, mm{carve.take<char>(sizes[1])}, steps{carve.take<char>(sizes[2])},
        pos{carve.take<char>(sizes[3])}, nextA{carve.take<char>(sizes[4])}, nextB{carve.take<char>(sizes[5])},
        nextC{carve.take<char>(sizes[6])}, reach{carve.take<char>(sizes[7])}, rank{carve.take<char>(sizes[8])},
        table{carve.take<char>(sizes[9])}, small{carve.take<char>(sizes[10])}, stage_idx{carve.take<char>(sizes[11])},
        atbuf{carve.take<char>(sizes[12])};
    uint32_t *d_small = small.as<uint32_t>();
    Rec *d_table = table.as<Rec>();

    std::vector<fs_la_stage_u32> stages;
    uint32_t la_size = 0;
    uint32_t h[4];

    // A few words from the device: through the mailbox (a tiny kernel writes them into coherent page-locked memory and then
    // a sequence number; the host spins on that word) -- or, if the mailbox could not be had or stays silent, the plain way
    if (!r->la_mail) {
        if (hipHostMalloc((void **)&r->la_mail, 32 * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            r->la_mail = nullptr;
        } else {
            memset(r->la_mail, 0, 32 * sizeof(uint32_t));
        }
    }
    auto read_words = [&](const uint32_t *src, uint32_t n, uint32_t *out) -> hipError_t {
        if (r->la_mail && n <= 31u) {
            const uint32_t seq = ++r->la_mail_seq ? r->la_mail_seq : ++r->la_mail_seq; // never 0
            fsk_la_mail(src, n, r->la_mail, seq, s);
            volatile uint32_t *m = r->la_mail;
            for (uint64_t spin = 0; spin < 400000000ull; spin++) { // (seconds; a launch error shows below)
                if (m[31] == seq) {
                    __atomic_thread_fence(__ATOMIC_ACQUIRE);
                    for (uint32_t i = 0; i < n; i++)
                        out[i] = m[i];
                    return hipSuccess;
                }
                if ((spin & 0xFFFFFu) == 0xFFFFFu && hipStreamQuery(s) != hipErrorNotReady)
                    break; // the stream has drained (or failed) without the word arriving: read the plain way
            }
        }
        hipError_t e = hipMemcpyAsync(out, src, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };

    // isZCoeffZero of the first step (LAReference.cpp:52-56): word 8 of the scratch words, read back with stage 0's first
    // detection below (one round trip less)
    fsk_la_tail<F>(zref, maxRef, nullptr, d_small + 8, s);

    // one stage: elements 0 .. limit-1 (+ the sentinel element `limit`), period / first record decided by the caller
    bool tail_written = false; // run_chain wrote the stage's tail record with its records
    auto run_chain = [&](bool stage0, const Rec *P, uint32_t limit, uint32_t period, bool have_first, uint32_t first_end,
                         uint32_t first_step, uint32_t x_start, uint32_t &n_records) -> uint32_t {
        const uint32_t nstates = 2u * limit; // limit <= maxRef < 2^31 - 1
        tail_written = false;
        uint32_t offset = 0;
        // room for this stage's first record and its tail record before anything is written
        if ((size_t)la_size + 2u > cap_recs)
            return FS_ERR_7;
        if (have_first) {
            fsk_la_one_record<F>(stage0, zref, P, first_end, first_step, d_table + la_size, s);
            offset = 1;
        }
        n_records = offset;
        if (x_start != kLaTerm && (x_start >> 1) < limit) {
            fsk_la_next<F>(stage0, chebv.p, mm.p, pos.as<uint32_t>(), limit, period, nextA.as<uint32_t>(), reach.as<uint32_t>(),
                           x_start, s); // (also zeroes reach and marks the chain's start)
            // jump tables ping-pong between nextB and nextC; the original next stays in nextA for the record kernel
            if (nstates <= (1u << 16)) {
                // a small stage: every round in one launch (the launches were most of the time on a small orbit)
                uint32_t rounds = 0;
                for (uint32_t span = 1; span < limit + 1u; span <<= 1)
                    rounds++;
                fsk_la_reach_all(nextA.as<uint32_t>(), nextB.as<uint32_t>(), nextC.as<uint32_t>(), reach.as<uint32_t>(), nstates,
                                 rounds, s);
            } else {
                uint32_t *jin = nextA.as<uint32_t>(), *jout = nextB.as<uint32_t>();
                for (uint32_t span = 1; span < limit + 1u; span <<= 1) {
                    fsk_la_reach(jin, jout, reach.as<uint32_t>(), nstates, s);
                    jin = jout;
                    jout = jout == nextB.as<uint32_t>() ? nextC.as<uint32_t>() : nextB.as<uint32_t>();
                }
            }
            fsk_scan_u32(reach.as<uint32_t>(), rank.as<uint32_t>(), nstates, s);
            FS_TRY(read_words(rank.as<uint32_t>() + nstates, 1, h));
            if ((size_t)la_size + offset + h[0] + 2u > cap_recs)
                return FS_ERR_7;
            // (the stage's tail record goes out with the same launch)
            fsk_la_records<F>(stage0, zref, P, pos.as<uint32_t>(), nextA.as<uint32_t>(), reach.as<uint32_t>(),
                              rank.as<uint32_t>(), limit, offset, d_table + la_size, d_table + la_size + offset + h[0], maxRef, s);
            n_records = offset + h[0];
            tail_written = true;
        }
        return (uint32_t)hipGetLastError();
    };

    // ---------------- stage 0: CreateLAFromOrbit, LAReference.cpp:28-210
    bool no_table = false; // CreateLAFromOrbit returned false: the records stay, the table is not valid
    {
        const uint32_t limit = maxRef;
        fsk_la_src_orbit<F>(zref, maxRef + 1u, chebv.p, s);
        fsk_la_first<F>(true, chebv.p, mm.p, limit, d_small, s);
        uint32_t h0[9];
        FS_TRY(read_words(d_small, 9, h0));
        if (h0[8])
            return FS_ERR_UNSUPPORTED; // the first step's ZCoeff is zero
        h[0] = h0[0], h[1] = h0[1];
        uint32_t Period = h[0] == kLaTerm ? 0u : h[0];
        bool have_first = false;
        uint32_t x_start;
        const double NthRoot = std::round(std::log2((double)maxRef) / periodDivisor);
        if (Period == 0 && maxRef <= kLaLowBound) {
            // :135-140: no period in an orbit of at most 64 steps -- one record over the whole orbit and the closing one,
            // CreateLAFromOrbit returns false and the table stays invalid (GenerateApproximationData, :1002-1005)
            no_table = true;
            x_start = kLaTerm;
        } else if (Period == 0 || Period > kLaLowBound) {
            Period = (uint32_t)std::round(std::pow((double)maxRef, 1.0 / NthRoot)); // :128-134 / :141-147
            x_start = 1u;                                                            // (0, flavour 1)
        } else {
            have_first = true; // the record that ended at the first detection stays (:97-101)
            const uint32_t i = Period;
            x_start = i + 1u < maxRef ? 2u * i + 1u : 2u * i; // :105-111: step z[i+1] at once unless that is the end
        }
        stages.push_back(fs_la_stage_u32{0u, 0u});
        uint32_t n = 0;
        // CreateLAFromOrbitMT (:215-770) is what the reference runs when the orbit has two or more 50 000-entry chunks and the
        // host two or more hardware threads (:236-251): the same prologue, then the scan in pieces
        size_t thread_count = maxRef / 50000u;
        if (thread_count > (size_t)(host_threads > 0 ? host_threads : 1))
            thread_count = (size_t)(host_threads > 0 ? host_threads : 1);
        if (no_table) {
            fsk_la_one_record<F>(true, zref, nullptr, maxRef, maxRef, d_table, s);
            n = 1;
            tail_written = false;
        } else if (thread_count > 1) {
            // Every piece of the reference's multi-threaded scan is a stretch of one of the chains x -> next(x) of the
            // single-threaded state machine: the Starter's from the prologue's state, Worker k's from the state its first
            // period detection leaves (two uncapped trackers begun one element apart at maxRef * k / N, :486-560); a piece ends
            // where its scan meets the start the next worker has published (:640-668, :440-470), and Stitch (:711-760) lines the
            // pieces up.  All cross-thread values are futures in the reference, so none of this depends on timing.  On the
            // device: next() for every state and the 2 (N - 1) first detections; the host walks the chains (indices only) and
            // stitches; the device folds the records of the segments that came out.
            const size_t TC = thread_count;
            const uint32_t nstates = 2u * limit;
            tail_written = false;
            if (have_first)
                fsk_la_one_record<F>(true, zref, nullptr, Period, Period, d_table, s);
            const uint32_t offset = have_first ? 1u : 0u;
            fsk_la_next<F>(true, chebv.p, mm.p, pos.as<uint32_t>(), limit, Period, nextA.as<uint32_t>(), reach.as<uint32_t>(), x_start, s);
            std::vector<uint32_t> bases(2u * (TC - 1u)), firsts(2u * (TC - 1u));
            for (size_t k = 1; k < TC; k++) {
                const uint32_t Begin = (uint32_t)((uint64_t)maxRef * k / TC);
                bases[2u * (k - 1u)] = Begin - 1u; // LA: z[Begin-1] stepped with z[Begin], tests from Begin + 1
                bases[2u * (k - 1u) + 1u] = Begin; // LA2: z[Begin] stepped with z[Begin+1], tests from Begin + 2
            }
            uint32_t *d_bases = nextB.as<uint32_t>(), *d_firsts = nextC.as<uint32_t>();
            FS_TRY(hipMemcpyAsync(d_bases, bases.data(), 4u * bases.size(), hipMemcpyHostToDevice, s));
            fsk_la_first_from<F>(chebv.p, d_bases, (uint32_t)bases.size(), limit, d_firsts, s);
            std::vector<uint32_t> hnext(nstates);
            FS_TRY(hipMemcpyAsync(firsts.data(), d_firsts, 4u * firsts.size(), hipMemcpyDeviceToHost, s));
            FS_TRY(hipMemcpyAsync(hnext.data(), nextA.p, 4u * (size_t)nstates, hipMemcpyDeviceToHost, s));
            FS_TRY(hipStreamSynchronize(s));
            FS_TRY(hipGetLastError());

            struct Piece {
                int64_t start = 0, finish = 0;
                std::vector<uint32_t> states; // the records this piece pushed: segment of state x = [x >> 1, next(x) >> 1)
                uint32_t last_b = 0, last_e = 0; // the record it was still accumulating when it stopped
            };
            std::vector<Piece> piece(TC);
            // the main scan of a piece (:392-484 Starter, :600-690 Worker): from state x; once past `end`, each boundary is
            // compared with the published start of the next piece
            auto walk = [&](uint32_t x, uint32_t end, size_t next_thread, Piece &pc) {
                for (;;) {
                    const uint32_t nx = hnext[x];
                    if (nx == kLaTerm) { // the scan ran to the end of the orbit: its open record covers the rest
                        pc.finish = maxRef;
                        pc.last_b = x >> 1, pc.last_e = maxRef;
                        return;
                    }
                    pc.states.push_back(x);
                    x = nx;
                    const uint32_t c = (x >> 1) + (x & 1u); // the scan index when the reference tests `j > End`
                    if (c > end && next_thread < TC) {
                        const int64_t ns = piece[next_thread].start;
                        if ((int64_t)c == ns - 1) { // joined: the open record is what the new state has taken so far
                            pc.finish = (int64_t)c + 1;
                            pc.last_b = x >> 1, pc.last_e = (x >> 1) + (x & 1u) + 1u;
                            return;
                        }
                        if ((int64_t)c >= ns)
                            next_thread++;
                    }
                }
            };
            for (size_t k = TC - 1u; k >= 1u; k--) {
                const uint32_t Begin = (uint32_t)((uint64_t)maxRef * k / TC), End = (uint32_t)((uint64_t)maxRef * (k + 1u) / TC);
                const uint32_t dA = firsts[2u * (k - 1u)], dB = firsts[2u * (k - 1u) + 1u];
                // the loop tests LA at Begin + 1 + t, then LA2 at Begin + 2 + t: the first to fire wins, LA on a tie
                uint32_t d = kLaTerm;
                if (dA != kLaTerm && (dB == kLaTerm || (uint64_t)dA - (Begin + 1u) <= (uint64_t)dB - (Begin + 2u)))
                    d = dA;
                else if (dB != kLaTerm)
                    d = dB;
                uint32_t x = kLaTerm;
                int64_t j = maxRef;
                if (d != kLaTerm) {
                    const uint32_t f = d + 1u < maxRef ? 1u : 0u; // :520-527, :541-549
                    x = 2u * d + f;
                    j = (int64_t)d + 1 + f;
                }
                Piece &pc = piece[k];
                if (k == TC - 1u || (j >= (int64_t)Begin && j < (int64_t)End)) {
                    pc.start = j;
                } else { // no period boundary inside its own chunk: the worker adopts the next one's start and contributes nothing
                    pc.start = piece[k + 1u].start;
                    pc.finish = -1;
                    continue;
                }
                if (x == kLaTerm) { // (last worker, nothing detected: no records, finish == start)
                    pc.finish = maxRef;
                    pc.last_b = Begin - 1u, pc.last_e = maxRef;
                    continue;
                }
                walk(x, End, k + 1u, pc);
            }
            walk(x_start, maxRef / (uint32_t)TC, 1u, piece[0]);

            // Stitch, :711-760
            std::vector<uint32_t> seg;
            auto append = [&](const Piece &pc) {
                for (uint32_t x : pc.states) {
                    seg.push_back(x >> 1);
                    seg.push_back(hnext[x] >> 1);
                }
            };
            append(piece[0]);
            size_t last_to_add = 0, index = 0, jj = 0;
            while (index < TC - 1u && piece[jj].finish > piece[index + 1u].start)
                index++;
            index++;
            for (; index < TC; index++) {
                append(piece[index]);
                if (piece[index].finish > piece[index].start)
                    last_to_add = index;
                jj = index;
                while (index < TC - 1u && piece[jj].finish > piece[index + 1u].start)
                    index++;
            }
            seg.push_back(piece[last_to_add].last_b);
            seg.push_back(piece[last_to_add].last_e);
            const uint32_t nseg = (uint32_t)(seg.size() / 2u);
            if ((size_t)offset + nseg + 2u > cap_recs || seg.size() > cap_states)
                return FS_ERR_7;
            FS_TRY(hipMemcpyAsync(nextB.p, seg.data(), 4u * seg.size(), hipMemcpyHostToDevice, s));
            fsk_la_records_list<F>(zref, nextB.as<uint32_t>(), nseg, d_table + offset, d_table + offset + nseg, maxRef, s);
            FS_TRY(hipStreamSynchronize(s)); // (seg lives on this stack frame)
            FS_TRY(hipGetLastError());
            n = offset + nseg;
            tail_written = true;
        } else if (uint32_t e = run_chain(true, nullptr, limit, Period, have_first, have_first ? Period : 0u,
                                          have_first ? Period : 0u, x_start, n))
            return e;
        stages[0].MacroItCount = n;
        la_size = n;
        if (!tail_written)
            fsk_la_tail<F>(zref, maxRef, d_table + la_size, nullptr, s);
        la_size++;
    }

    // ---------------- higher stages: CreateNewLAStage, LAReference.cpp:774-966
    while (!no_table) {
        const uint32_t PrevStage = (uint32_t)stages.size() - 1u, CurrentStage = (uint32_t)stages.size();
        if (CurrentStage >= kLaMaxStages)
            break;
        const uint32_t PrevIdx = stages[PrevStage].LAIndex, Count = stages[PrevStage].MacroItCount;
        const Rec *P = d_table + PrevIdx;
        fsk_la_src_stage<F>(P, Count + 1u, chebv.p, mm.p, steps.as<uint32_t>(), s);
        // scan of the step lengths, first detection and everything the period decision reads: one launch, one read-back
        // (round 4: three launches and three round trips per stage before)
        fsk_la_stage_prologue<F>(P, chebv.p, mm.p, steps.as<uint32_t>(), pos.as<uint32_t>(), Count, d_small, s);
        uint32_t hs[5];
        FS_TRY(read_words(d_small, 5, hs));
        uint32_t jd = hs[0], fd = hs[1];
        const uint32_t step0 = hs[2];
        uint32_t Period = 0;
        if (jd != kLaTerm) {
            if (hs[4]) // isLAThresholdZero: the prologue breaks without a period (:815-817)
                jd = kLaTerm;
            else
                Period = hs[3];
        }
        stages.push_back(fs_la_stage_u32{la_size, 0u});
        const double NthRoot = std::round(std::log2((double)maxRef) / periodDivisor);
        bool have_first = false, last_stage = false;
        uint32_t x_start = 1u, first_end = 0, first_step = 0;
        if (Period == 0) {
            if ((uint64_t)maxRef > (uint64_t)step0 * kLaLowBound) {
                const double Ratio = ((double)maxRef) / step0;
                Period = step0 * (uint32_t)std::round(std::pow(Ratio, 1.0 / NthRoot)); // :861-869
            } else {
                // :870-881: one record over the whole previous stage, and this is the last stage
                last_stage = true;
                have_first = true;
                first_end = Count;
                first_step = maxRef;
                x_start = kLaTerm;
            }
        } else if ((uint64_t)Period > (uint64_t)step0 * kLaLowBound) {
            const double Ratio = ((double)Period) / step0;
            Period = step0 * ((uint32_t)std::round(std::pow(Ratio, 1.0 / NthRoot))); // :882-893
        } else {
            have_first = true;
            first_end = jd;
            first_step = Period;
            x_start = 2u * jd + fd;
        }
        uint32_t n = 0;
        if (uint32_t e = run_chain(false, P, Count, Period, have_first, first_end, first_step, x_start, n))
            return e;
        stages[CurrentStage].MacroItCount = last_stage ? 1u : n;
        la_size += n;
        if (!tail_written)
            fsk_la_tail<F>(zref, maxRef, d_table + la_size, nullptr, s);
        la_size++;
        if (last_stage)
            break;
    }

    // ---------------- CreateATFromLA + install
    const uint32_t stage_count = (uint32_t)stages.size();
    std::vector<uint32_t> idx(stage_count);
    for (uint32_t k = 0; k < stage_count; k++)
        idx[k] = stages[k].LAIndex;
    FS_TRY(hipMemcpyAsync(stage_idx.p, idx.data(), 4u * stage_count, hipMemcpyHostToDevice, s));
    if (!no_table)
        fsk_la_at<F>(d_table, stage_idx.as<uint32_t>(), stage_count, max_radius, use_small_exponents, atbuf.p, d_small, s);
    else { // (no CreateATFromLA: the ATInfo stays as constructed and is never used)
        FS_TRY(hipMemsetAsync(atbuf.p, 0, sizeof(fs::la::ATInfoT<F>), s));
        FS_TRY(hipMemsetAsync(d_small, 0, 4, s));
    }
    fs::la::ATInfoT<F> at;
    r->la_ok = false;
    const size_t rec_bytes = sizeof(F) == 4 ? sizeof(fs_la_hdr32_u32) : sizeof(fs_la_hdr64_u32);
    FS_TRY(la_reserve(r, rec_bytes * la_size, sizeof(fs_la_stage_u32) * stage_count));
    fsk_la_pack(sizeof(F) == 8, d_table, r->las.p, la_size, s);
    FS_TRY(hipMemcpyAsync(r->stages.p, stages.data(), sizeof(fs_la_stage_u32) * stage_count, hipMemcpyHostToDevice, s));
    FS_TRY(hipMemcpyAsync(&at, atbuf.p, sizeof(at), hipMemcpyDeviceToHost, s));
    FS_TRY(hipMemcpyAsync(h, d_small, 4, hipMemcpyDeviceToHost, s));
    FS_TRY(hipStreamSynchronize(s)); // (one round trip for the AT record, its flag, and the host temporaries above)
    FS_TRY(hipGetLastError());
    r->n_las = la_size;
    r->n_stages = stage_count;
    r->la_valid = no_table ? 0 : 1;
    r->use_at = !no_table && h[0] ? 1 : 0;
    memset(&r->at, 0, sizeof(r->at));
    memset(&r->at64, 0, sizeof(r->at64));
    if (!no_table)
        pack_at<F>(at, r);
    r->la_type = sizeof(F) == 4 ? FS_T_HDR32 : FS_T_HDR64;
    r->la_gen = 0;
    r->la_u64 = false; // the table just installed has uint32 fields, whatever an earlier fs_upload_la left behind
    r->at_step_hi = 0;
    r->la_ok = true;
    return 0;
}

} // namespace

extern "C" {

uint32_t fs_build_la(fs_renderer *r, int type_tag, const void *max_radius, int use_small_exponents)
{
    return fs_build_la_mt(r, type_tag, max_radius, use_small_exponents, 1);
}

uint32_t fs_build_la_mt(fs_renderer *r, int type_tag, const void *max_radius, int use_small_exponents, int host_threads)
{
    if (uint32_t e = use_device(r))
        return e;
    if (type_tag != FS_T_HDR32 && type_tag != FS_T_HDR64)
        return FS_ERR_UNSUPPORTED;
    if (!r->compute || !r->orbit_ok || r->orbit_type != type_tag || !max_radius)
        return FS_ERR_6;
    if (r->orbit_seq)
        return FS_ERR_UNSUPPORTED; // needs the expanded orbit (fs_set_compressed_orbit_mode 0)
    TimedLaunch t(r);
    return type_tag == FS_T_HDR32 ? build_la<float>(r, max_radius, use_small_exponents, host_threads)
                                  : build_la<double>(r, max_radius, use_small_exponents, host_threads);
}

} // extern "C"
