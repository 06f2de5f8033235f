// inputs_dump.cpp -- every product of the host input builders (C ABI: include/fs_inputs.h) for one view, as one line each:
//     name  byte_count  fnv1a64
// Two builds of fractalshark_amd/host/ compute the same inputs exactly when their dumps are equal line for line.  The program
// uses the C ABI alone and is compiled together with host/*.cpp (tools/dump_host_inputs.py), not against libfsinputs.so.
//
//     inputs_dump minX minY maxX maxY width height iteration_cap [long_orbit_cap]
//
// long_orbit_cap (optional): one more HDRFloat<float> orbit without periodicity up to that many iterations, and its LAv2 table for
// 1 and 8 host threads -- the multi-threaded stage-0 scan only starts at 100 000 orbit entries.
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fs_inputs.h"

namespace {

// (an empty product prints no line: every line of a dump has bytes behind its hash)
void put(const std::string &name, const void *data, size_t bytes)
{
    if (bytes == 0)
        return;
    uint64_t h = 0xcbf29ce484222325ull; // FNV-1a 64
    for (size_t i = 0; i < bytes; i++)
        h = (h ^ ((const unsigned char *)data)[i]) * 0x100000001b3ull;
    printf("%s  %zu  %016llx\n", name.c_str(), bytes, (unsigned long long)h);
}
template <class T> void put_val(const std::string &name, T v) { put(name, &v, sizeof v); }
template <class T> void put_vec(const std::string &name, const std::vector<T> &v) { put(name, v.data(), v.size() * sizeof(T)); }

struct TempFile {
    char path[64];
    TempFile()
    {
        strcpy(path, "/tmp/inputs_dump_XXXXXX");
        const int fd = mkstemp(path);
        if (fd < 0) {
            perror("mkstemp");
            exit(2);
        }
        close(fd);
    }
    ~TempFile() { unlink(path); }
    void put_bytes(const std::string &name) const
    {
        std::vector<unsigned char> b;
        if (FILE *f = fopen(path, "rb")) {
            unsigned char buf[65536];
            for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
                b.insert(b.end(), buf, buf + n);
            fclose(f);
        }
        put_vec(name, b);
    }
};

uint32_t W, H;

void dump_view(const std::string &p, const fsh_view *v)
{
    put_val(p + ".precision_bits", fsh_view_precision_bits(v));
    for (int k = 0; k < 4; k++) {
        char one[1];
        const int n = fsh_view_bbox_str(v, k, one, sizeof one);
        std::string s((size_t)n + 1, '\0');
        fsh_view_bbox_str(v, k, &s[0], s.size());
        put(p + ".bbox" + std::to_string(k), s.data(), (size_t)n);
    }
    fs_real_hdr32 c32[4];
    fs_real_hdr64 c64[4];
    double cd[4];
    memset(c64, 0, sizeof c64);
    fsh_view_coords_direct_hdr32(v, W, H, c32);
    fsh_view_coords_direct_hdr64(v, W, H, c64);
    fsh_view_coords_direct_f64(v, W, H, cd);
    put(p + ".coords_direct_hdr32", c32, sizeof c32);
    put(p + ".coords_direct_hdr64", c64, sizeof c64);
    put(p + ".coords_direct_f64", cd, sizeof cd);
    const size_t lp_bytes[5] = {16, 32, 64, 64, 128};
    for (int kind = 0; kind < 5; kind++) {
        unsigned char out[128] = {0};
        fsh_view_coords_direct_lp(v, W, H, kind, out);
        put(p + ".coords_direct_lp" + std::to_string(kind), out, lp_bytes[kind]);
    }
}

void dump_exact_axes(const fsh_view *v)
{
    const uint32_t frac_bits = 96, limbs = 4;
    for (int shift = 0; shift <= 1; shift++) {
        std::vector<uint32_t> cx(3u * limbs * W, 0), cy(3u * limbs * H, 0);
        const int rc = fsh_view_exact_axes(v, W, H, frac_bits, shift, limbs, cx.data(), cy.data());
        const std::string p = "exact_axes.s" + std::to_string(shift);
        put_val(p + ".rc", rc);
        put_vec(p + ".cx", cx);
        put_vec(p + ".cy", cy);
    }
}

void dump_la(const std::string &p, const fsh_la *l)
{
    const int is64 = fsh_la_is64(l);
    const uint32_t n = fsh_la_count(l);
    put_val(p + ".count", n);
    put(p + ".records", fsh_la_data(l), (size_t)n * (is64 ? sizeof(fs_la_hdr64_u32) : sizeof(fs_la_hdr32_u32)));
    put(p + ".stages", fsh_la_stages(l), (size_t)fsh_la_stage_count(l) * sizeof(fs_la_stage_u32));
    put_val(p + ".valid", fsh_la_is_valid(l));
    put_val(p + ".use_at", fsh_la_use_at(l));
    if (is64) {
        fs_at_hdr64_u32 at;
        fsh_la_at(l, &at);
        put_val(p + ".at", at);
        std::vector<fs_la_2x32_u32> c(n);
        fsh_convert_la_hdr64_to_2x32((const fs_la_hdr64_u32 *)fsh_la_data(l), n, c.data());
        put_vec(p + ".records_2x32", c);
        fs_at_2x32_u32 at2;
        fsh_convert_at_hdr64_to_2x32(&at, &at2);
        put_val(p + ".at_2x32", at2);
    } else {
        fs_at_hdr32_u32 at;
        fsh_la_at(l, &at);
        put_val(p + ".at", at);
    }
}

void dump_bla_levels(const std::string &p, int32_t levels, int32_t lm2, const void *const *ptrs, const uint64_t *sizes, size_t rec)
{
    put_val(p + ".num_levels", levels);
    put_val(p + ".lm2", lm2);
    put(p + ".sizes", sizes, (size_t)levels * sizeof(uint64_t));
    for (int32_t l = 0; l < levels; l++)
        if (sizes[l])
            put(p + ".level" + std::to_string(l), ptrs[l], (size_t)sizes[l] * rec);
}

// tables: the LAv2 table for host threads 1 / 8 x small exponents 0 / 1, and the BLA table
void dump_orbit(const std::string &p, const fsh_view *v, fsh_orbit *o, bool tables)
{
    const int is64 = fsh_orbit_is64(o);
    const uint64_t n = fsh_orbit_count(o);
    put_val(p + ".count", n);
    put_val(p + ".period", fsh_orbit_period(o));
    put_val(p + ".bad_count", fsh_orbit_bad_count(o));
    fs_real_2x32 low2[2], c2[4];
    fsh_orbit_low_2x32(o, low2);
    fsh_view_coords_perturb_2x32(v, o, W, H, c2);
    put(p + ".orbit_low_2x32", low2, sizeof low2);
    put(p + ".coords_perturb_2x32", c2, sizeof c2);
    if (is64) {
        put(p + ".data", fsh_orbit_data_hdr64(o), n * sizeof(fs_orbit_hdr64));
        std::vector<fs_orbit_2x32> c(n);
        fsh_convert_orbit_hdr64_to_2x32(fsh_orbit_data_hdr64(o), n, c.data());
        put_vec(p + ".data_2x32", c);
        fs_real_hdr64 low[2], r, co[4];
        fsh_orbit_low_hdr64(o, low);
        fsh_orbit_max_radius_hdr64(o, &r);
        fsh_view_coords_perturb_hdr64(v, o, W, H, co);
        put(p + ".orbit_low", low, sizeof low);
        put_val(p + ".max_radius", r);
        put(p + ".coords_perturb", co, sizeof co);
        if (fsh_orbit_is_compressed(o)) {
            const uint64_t k = fsh_orbit_compressed_count(o);
            put(p + ".waypoints", fsh_orbit_compressed_data_hdr64(o), k * sizeof(fs_orbit_hdr64_rc));
            std::vector<fs_orbit_2x32_rc> rc(k);
            fsh_convert_orbit_rc_hdr64_to_2x32(fsh_orbit_compressed_data_hdr64(o), k, rc.data());
            put_vec(p + ".waypoints_2x32", rc);
        }
    } else {
        put(p + ".data", fsh_orbit_data_hdr32(o), n * sizeof(fs_orbit_hdr32));
        put(p + ".data_hdr32_bad", fsh_orbit_data_hdr32_bad(o), n * sizeof(fs_orbit_hdr32_bad));
        put(p + ".data_f32_bad", fsh_orbit_data_f32_bad(o), n * sizeof(fs_orbit_f32_bad));
        fs_real_hdr32 low[2], r, co[4];
        fsh_orbit_low_hdr32(o, low);
        fsh_orbit_max_radius_hdr32(o, &r);
        fsh_view_coords_perturb_hdr32(v, o, W, H, co);
        put(p + ".orbit_low", low, sizeof low);
        put_val(p + ".max_radius", r);
        put(p + ".coords_perturb", co, sizeof co);
        if (fsh_orbit_is_compressed(o))
            put(p + ".waypoints", fsh_orbit_compressed_data_hdr32(o), fsh_orbit_compressed_count(o) * sizeof(fs_orbit_hdr32_rc));
    }
    if (!tables)
        return;
    for (int threads : {1, 8})
        for (int small : {0, 1}) {
            fsh_la *l = fsh_la_create_ex(o, threads, small);
            dump_la(p + ".la.t" + std::to_string(threads) + ".s" + std::to_string(small), l);
            fsh_la_destroy(l);
        }
    fsh_bla *b = fsh_bla_create(o);
    dump_bla_levels(p + ".bla", fsh_bla_num_levels(b), fsh_bla_lm2(b), fsh_bla_level_ptrs(b), fsh_bla_level_sizes(b),
                    is64 ? sizeof(fs_bla_hdr64) : sizeof(fs_bla_hdr32));
    fsh_bla_destroy(b);
}

void dump_orbit_f64(const std::string &p, const fsh_view *v, fsh_orbit_f64 *o)
{
    const uint64_t n = fsh_orbit_f64_count(o);
    put_val(p + ".count", n);
    put_val(p + ".period", fsh_orbit_f64_period(o));
    put(p + ".data", fsh_orbit_f64_data(o), n * sizeof(fs_orbit_f64));
    put(p + ".data_bad", fsh_orbit_f64_data_bad(o), n * sizeof(fs_orbit_f64_bad));
    put(p + ".data_f32_bad", fsh_orbit_f64_data_f32_bad(o), n * sizeof(fs_orbit_f32_bad));
    std::vector<fs_orbit_p2x32> c(n);
    fsh_convert_orbit_f64_to_p2x32(fsh_orbit_f64_data(o), n, c.data());
    put_vec(p + ".data_p2x32", c);
    dump_bla_levels(p + ".bla", fsh_orbit_f64_bla_num_levels(o), fsh_orbit_f64_bla_lm2(o), fsh_orbit_f64_bla_level_ptrs(o),
                    fsh_orbit_f64_bla_level_sizes(o), sizeof(fs_bla_f64));
    double co[4];
    fsh_view_coords_perturb_f64(v, o, W, H, co);
    put(p + ".coords_perturb", co, sizeof co);
}

void dump_plain(const std::string &p, const fsh_view *v, const fsh_plain *h)
{
    const int kind = fsh_plain_kind(h);
    const uint64_t n = fsh_plain_orbit_count(h), k = fsh_plain_compressed_count(h);
    const uint32_t nla = fsh_plain_la_count(h);
    put_val(p + ".count", n);
    put_val(p + ".period", fsh_plain_orbit_period(h));
    put(p + ".data", fsh_plain_orbit_data(h), n * (kind ? sizeof(fs_orbit_f64) : sizeof(fs_orbit_f32)));
    put_val(p + ".compressed", fsh_plain_is_compressed(h));
    put(p + ".waypoints", fsh_plain_compressed_data(h), k * (kind ? sizeof(fs_orbit_f64_rc) : sizeof(fs_orbit_f32_rc)));
    double low[2] = {0, 0}, co[4] = {0, 0, 0, 0};
    fsh_plain_orbit_low(h, low);
    fsh_plain_coords(v, h, W, H, co);
    put(p + ".orbit_low", low, kind ? 16 : 8);
    put(p + ".coords", co, kind ? 32 : 16);
    put(p + ".la.records", fsh_plain_la_data(h), (size_t)nla * (kind ? sizeof(fs_la_f64_u32) : sizeof(fs_la_f32_u32)));
    put(p + ".la.stages", fsh_plain_la_stages(h), (size_t)fsh_plain_la_stage_count(h) * sizeof(fs_la_stage_u32));
    put_val(p + ".la.valid", fsh_plain_la_is_valid(h));
    put_val(p + ".la.use_at", fsh_plain_la_use_at(h));
    unsigned char at[sizeof(fs_at_f64_u32)] = {0};
    fsh_plain_la_at(h, at);
    put(p + ".la.at", at, kind ? sizeof(fs_at_f64_u32) : sizeof(fs_at_f32_u32));
    if (kind) { // the Gpu2x32PerturbedLAv2* inputs: converted field-wise from the double ones
        std::vector<fs_orbit_p2x32> o2(n);
        std::vector<fs_orbit_p2x32_rc> w2(k);
        std::vector<fs_la_p2x32_u32> l2(nla);
        fs_at_p2x32_u32 a2;
        fs_real_p2x32 c2[4];
        fsh_convert_orbit_f64_to_p2x32((const fs_orbit_f64 *)fsh_plain_orbit_data(h), n, o2.data());
        fsh_convert_orbit_rc_f64_to_p2x32((const fs_orbit_f64_rc *)fsh_plain_compressed_data(h), k, w2.data());
        fsh_convert_la_f64_to_p2x32((const fs_la_f64_u32 *)fsh_plain_la_data(h), nla, l2.data());
        fsh_convert_at_f64_to_p2x32((const fs_at_f64_u32 *)at, &a2);
        fsh_convert_coords_f64_to_p2x32(co, c2);
        put_vec(p + ".data_p2x32", o2);
        put_vec(p + ".waypoints_p2x32", w2);
        put_vec(p + ".la.records_p2x32", l2);
        put_val(p + ".la.at_p2x32", a2);
        put(p + ".coords_p2x32", c2, sizeof c2);
    }
}

// the first batch of a scan, no evaluation results fed back
void dump_feature_batch(const std::string &p, fsh_feature *f)
{
    const int is64 = fsh_feature_is64(f);
    const uint64_t cands = fsh_feature_candidates(f);
    std::vector<unsigned char> in(cands * sizeof(fs_feature_in_hdr64), 0);
    fs_real_hdr64 radius;
    memset(&radius, 0, sizeof radius);
    int mode = -1;
    uint64_t max_iters = 0;
    const uint64_t n = fsh_feature_next_batch(f, in.data(), cands, &mode, &radius, &max_iters);
    put_val(p + ".candidates", cands);
    put_val(p + ".batch", n);
    put_val(p + ".mode", mode);
    put_val(p + ".max_iters", max_iters);
    put(p + ".radius", &radius, is64 ? sizeof(fs_real_hdr64) : sizeof(fs_real_hdr32));
    put(p + ".records", in.data(), n * (is64 ? sizeof(fs_feature_in_hdr64) : sizeof(fs_feature_in_hdr32)));
    fsh_feature_destroy(f);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 8 && argc != 9) {
        fprintf(stderr, "usage: %s minX minY maxX maxY width height iteration_cap [long_orbit_cap]\n", argv[0]);
        return 2;
    }
    W = (uint32_t)strtoul(argv[5], nullptr, 10), H = (uint32_t)strtoul(argv[6], nullptr, 10);
    const uint64_t cap = strtoull(argv[7], nullptr, 10), long_cap = argc == 9 ? strtoull(argv[8], nullptr, 10) : 0;
    fsh_view *v = fsh_view_create(argv[1], argv[2], argv[3], argv[4], W, H);
    dump_view("view", v);
    dump_exact_axes(v);
    {
        fsh_view *nv = fsh_view_autozoom_next(v, W / 3.0, H / 4.0, W, H, 3);
        dump_view("view.autozoom_next", nv);
        fsh_view_destroy(nv);
    }
    {
        int32_t params[7];
        fsh_la_default_params(params);
        put("la_default_params", params, sizeof params);
        unsigned char raw[64] = {0};
        char dec[64] = {0};
        const size_t wrote = fsh_mpz_raw_write("-123456789012345678901234567890", 10, raw, sizeof raw);
        put("mpz_raw.write", raw, wrote);
        put_val("mpz_raw.read", fsh_mpz_raw_read(raw, wrote, dec, sizeof dec));
        put("mpz_raw.decimal", dec, strlen(dec));
    }
    for (int exp_bytes : {4, 8}) {
        TempFile t;
        const std::string p = "view.im" + std::to_string(exp_bytes);
        put_val(p + ".save_rc", fsh_view_save_im(v, cap, t.path, exp_bytes));
        t.put_bytes(p + ".file");
        uint64_t limit = 0;
        int has_orbit = -1, eb = -1;
        // (a view too deep for a double radius has no location form to load: NULL, like the reference)
        fsh_view *lv = fsh_view_load_im(t.path, W, H, &limit, &has_orbit, &eb);
        put_val(p + ".loaded", lv ? 1 : 0);
        if (lv) {
            put_val(p + ".limit", limit);
            put_val(p + ".has_orbit", has_orbit);
            put_val(p + ".exp_bytes", eb);
            dump_view(p + ".load", lv);
            fsh_view_destroy(lv);
        }
    }
    for (int is64 : {0, 1})
        for (int periodicity : {1, 0})
            for (int comp : {-1, 20}) {
                fsh_orbit *o = fsh_orbit_create_ex(v, is64, cap, periodicity, comp);
                const std::string p = std::string("orbit.") + (is64 ? "hdr64" : "hdr32") + ".p" + std::to_string(periodicity) + ".c" +
                                      std::to_string(comp);
                dump_orbit(p, v, o, true);
                if (periodicity && comp < 0) {
                    TempFile t;
                    put_val(p + ".im.save_rc", fsh_orbit_save_im(o, cap, 20, t.path, 8));
                    t.put_bytes(p + ".im.file");
                    uint64_t limit = 0;
                    fsh_orbit *lo = fsh_orbit_load_im(t.path, &limit);
                    put_val(p + ".im.loaded", lo ? 1 : 0);
                    if (lo) {
                        put_val(p + ".im.limit", limit);
                        dump_orbit(p + ".im.load", v, lo, true);
                        fsh_orbit_destroy(lo);
                    }
                    for (int direct : {0, 1})
                        dump_feature_batch(p + (direct ? ".feature_direct" : ".feature"),
                                           direct ? fsh_feature_begin_direct(v, is64, 4, 4, 4, cap) : fsh_feature_begin(v, o, 4, 4, 4, cap));
                    dump_feature_batch(p + ".feature_direct_at", fsh_feature_begin_direct_at(v, is64, W / 2, H / 2, 8, cap));
                    std::vector<unsigned char> in(16 * sizeof(fs_feature_in_hdr64), 0);
                    fs_real_hdr64 radius;
                    memset(&radius, 0, sizeof radius);
                    put_val(p + ".feature_direct_grid.rc", fsh_feature_direct_grid(v, is64, 4, 4, in.data(), &radius));
                    put(p + ".feature_direct_grid.radius", &radius, is64 ? sizeof(fs_real_hdr64) : sizeof(fs_real_hdr32));
                    put(p + ".feature_direct_grid.records", in.data(), 16 * (is64 ? sizeof(fs_feature_in_hdr64) : sizeof(fs_feature_in_hdr32)));
                }
                fsh_orbit_destroy(o);
            }
    if (long_cap) {
        fsh_orbit *o = fsh_orbit_create_ex(v, 0, long_cap, 0, -1);
        dump_orbit("orbit.long", v, o, false);
        for (int threads : {1, 8}) {
            fsh_la *l = fsh_la_create(o, threads);
            dump_la("orbit.long.la.t" + std::to_string(threads), l);
            fsh_la_destroy(l);
        }
        fsh_orbit_destroy(o);
    }
    for (int periodicity : {1, 0}) {
        fsh_orbit_f64 *o = fsh_orbit_f64_create(v, cap, periodicity);
        dump_orbit_f64("orbit_f64.p" + std::to_string(periodicity), v, o);
        fsh_orbit_f64_destroy(o);
    }
    for (int kind : {0, 1})
        for (int comp : {-1, 20}) {
            fsh_plain *h = fsh_plain_create_ex(v, kind, cap, 1, 8, comp);
            const std::string p = std::string("plain.") + (kind ? "f64" : "f32") + ".c" + std::to_string(comp);
            dump_plain(p, v, h);
            if (comp < 0) {
                TempFile t;
                put_val(p + ".im.save_rc", fsh_plain_save_im(h, cap, 20, t.path, 4));
                t.put_bytes(p + ".im.file");
                uint64_t limit = 0;
                fsh_plain *lh = fsh_plain_load_im(t.path, &limit, 8);
                put_val(p + ".im.loaded", lh ? 1 : 0);
                if (lh) {
                    put_val(p + ".im.limit", limit);
                    dump_plain(p + ".im.load", v, lh);
                    fsh_plain_destroy(lh);
                }
            }
            fsh_plain_destroy(h);
        }
    fsh_view_destroy(v);
    return 0;
}
