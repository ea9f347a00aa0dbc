// The scan-line planner (scan_plan.h) on the CPU: no HIP, no device, never loaded into Python.  Built by `make scan_plan_check`
// (SAN=1: with the address and undefined-behaviour sanitizers); tests/test_cpu_scan_plan.py drives both modes.
//
//   scan_plan_check replay < lines     one answer line per input line:
//       geometry <channels> <ctx_out> <ksize> <prior_channels> <n_dense> <dense_out ...> <act_after ... (n_dense + 1)> <in_groups ...>
//           -> "geometry <nwg> <weight_floats> <batched 0|1> <b_nw>"; the lines after it are asked of this geometry
//       limits <h> <w> <compute units>
//           -> "limits <batched_max encode> <batched_max decode> <wavefront_max> <band_max>" (what basic_scanline_*_max report)
//       limits-decode <h> <w> <lanes> <compute units>
//           -> "limits-decode <band_decode_max>" (what basic_scanline_band_decode_max reports for a table set whose search image fits)
//       call <batch> <h> <w> <encode|decode> <auto|raster|wavefront|band> <none|a BASIC_SCAN_KERNEL spelling> <lane_max_batch> <lanes>
//            <rows 0|1> <table_len> <decoder_lds> <compute units> [<decode schedule: auto|raster|wavefront|band>]
//           -> "<kernel's spelling | per-step | raises> <launches> <the refusal's text>"; a decode call has a fast search image
//   scan_plan_check sweep < geometry lines
//       plans a fixed list of requests for every geometry and checks what the spin-wait protocol rests on (see sweep());
//       prints the first offending requests and exits 1 on any violation.
//   scan_plan_check sweep-decode < geometry lines
//       the same for row-stream decode requests over every decode schedule (the list sweep() keeps fixed has none but auto).
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "scan_plan.h"

namespace basic {
static std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
}  // namespace basic

using namespace basic;

namespace {

const char *const kSchedules[] = {"auto", "raster", "wavefront", "band"};   // BASIC_SCAN_SCHEDULE_*
constexpr int kKernels = static_cast<int>(ScanKernel::kNone);

bool read_geometry(std::istream &in, ScanGeometry *g)
{
    int channels = 0, ctx_out = 0, ksize = 0, prior = 0, n = 0;
    int outs[kMaxLayers] = {}, acts[kMaxLayers] = {}, groups[kMaxLayers] = {};
    if (!(in >> channels >> ctx_out >> ksize >> prior >> n) || n < 1 || n > kMaxLayers - 1) return false;
    for (int l = 0; l < n; ++l) in >> outs[l];
    for (int l = 0; l <= n; ++l) in >> acts[l];
    for (int l = 0; l < n; ++l) in >> groups[l];
    if (!in) return false;
    if (scan_geometry(channels, ctx_out, ksize, prior, n, outs, acts, groups, g)) {
        fprintf(stderr, "scan_plan_check: %s\n", g_error.c_str());
        return false;
    }
    return true;
}

int index_of(const std::string &s, const char *const *names, int n)
{
    for (int i = 0; i < n; ++i)
        if (s == names[i]) return i;
    return -1;
}

int replay()
{
    ScanGeometry g;
    bool have = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "geometry") {
            have = read_geometry(in, &g);
            if (!have) { fprintf(stderr, "scan_plan_check: bad geometry line: %s\n", line.c_str()); return 2; }
            printf("geometry %d %d %d %d\n", g.nwg, g.weight_floats, g.batched ? 1 : 0, g.b_nw);
            continue;
        }
        if (!have) { fprintf(stderr, "scan_plan_check: no geometry before: %s\n", line.c_str()); return 2; }
        if (what == "limits") {
            int h = 0, w = 0, cus = 0;
            if (!(in >> h >> w >> cus)) { fprintf(stderr, "scan_plan_check: bad line: %s\n", line.c_str()); return 2; }
            printf("limits %d %d %d %d\n", batched_max_batch(&g, w, false, cus), batched_max_batch(&g, w, true, cus), wavefront_max_batch(&g, h, cus),
                   band_images_per_launch(&g, h, w, cus));
            continue;
        }
        if (what == "limits-decode") {
            int h = 0, w = 0, lanes = 0, cus = 0;
            if (!(in >> h >> w >> lanes >> cus)) { fprintf(stderr, "scan_plan_check: bad line: %s\n", line.c_str()); return 2; }
            printf("limits-decode %d\n", valid_lanes(&g, lanes) ? band_decode_images_per_launch(&g, h, w, lanes, cus) : 0);
            continue;
        }
        ScanRequest q;
        std::string direction, schedule, force, decode_schedule;
        int rows = 0;
        long long decoder_lds = 0;
        if (what != "call" || !(in >> q.batch >> q.h >> q.w >> direction >> schedule >> force >> q.lane_max_batch >> q.lanes >> rows >> q.table_len >>
                                decoder_lds >> q.cus)) {
            fprintf(stderr, "scan_plan_check: bad line: %s\n", line.c_str());
            return 2;
        }
        const char *envs[kKernels];
        for (int k = 0; k < kKernels; ++k) envs[k] = kScanKernelNames[k].env;
        q.schedule = index_of(schedule, kSchedules, 4);
        if (in >> decode_schedule) q.decode_schedule = index_of(decode_schedule, kSchedules, 4);   // (optional: auto when it is not there)
        const int forced = index_of(force, envs, kKernels);
        if ((direction != "encode" && direction != "decode") || q.schedule < 0 || q.decode_schedule < 0 || (forced < 0 && force != "none")) {
            fprintf(stderr, "scan_plan_check: bad name in: %s\n", line.c_str());
            return 2;
        }
        q.force = forced < 0 ? ScanKernel::kNone : static_cast<ScanKernel>(forced);
        q.decode = direction == "decode";
        q.fast_image = q.decode;
        q.decoder_lds = q.decode ? static_cast<size_t>(decoder_lds) : 0;
        q.rows = rows != 0 && q.decode;
        ScanLaunch L;
        g_error.clear();
        if (plan_scan(&g, q, &L)) printf("raises 0 %s\n", g_error.c_str());
        else if (L.kernel == ScanKernel::kNone) printf("per-step 0\n");
        else printf("%s %d\n", kScanKernelNames[static_cast<int>(L.kernel)].env, L.launches);
    }
    return 0;
}

// Every planned launch must be resident and complete: launches >= 1 over images >= 1 whole images each, launches = ceil(batch /
// images); 1 <= grid <= compute units (one workgroup per unit, or the spin-waits never end); kMinLds <= lds_bytes <= kMaxLds (more
// than half a unit's LDS, so no second workgroup joins it).  A library call (lane_max_batch < 0) is served or refused, never left
// to the per-step path.  Requests the entry points refuse before they plan are not made: lane counts that are not valid_lanes,
// lanes or rows on an encode call, a library call of unknown shape.
// decode_only: the row-stream decode requests alone, over every decode schedule (at the encode schedule auto, which decode calls
// ignore); otherwise the list as it always was, every request at the decode schedule auto.
int sweep(bool decode_only)
{
    static const int shapes[][2] = {{0, 0}, {1, 1}, {1, 4}, {2, 2}, {3, 2}, {4, 3}, {4, 4}, {5, 5}, {16, 16}, {32, 48}, {48, 32}, {70, 24}, {3, 130},
                                    {135, 120}, {64, 1}, {1, 200}};
    static const int batches[] = {1, 2, 3, 4, 5, 8, 13, 16, 32, 33, 64, 65, 96, 100};
    static const int units[] = {64, 256, 304}, lane_counts[] = {1, 3, 12}, gates[] = {-1, 4};
    long requests = 0, planned = 0, refused = 0, per_step = 0, violations = 0;
    std::string line;
    int geometries = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        ScanGeometry g;
        if (what != "geometry" || !read_geometry(in, &g)) { fprintf(stderr, "scan_plan_check: bad geometry line: %s\n", line.c_str()); return 2; }
        ++geometries;
        for (int cus : units) for (const auto &s : shapes) for (int batch : batches) for (int decode = decode_only ? 1 : 0; decode < 2; ++decode)
        for (int schedule = BASIC_SCAN_SCHEDULE_AUTO; schedule <= BASIC_SCAN_SCHEDULE_BAND; ++schedule) for (int force = 0; force <= kKernels; ++force)
        for (int gate : gates) for (int lanes : lane_counts) for (int rows = decode_only ? 1 : 0; rows < 2; ++rows) {
            if (!valid_lanes(&g, lanes) || (!decode && (lanes > 1 || rows)) || (gate < 0 && s[0] < 1)) continue;
            ScanRequest q;
            // (sweep-decode: the loop over the four schedules walks the DECODE schedule)
            if (decode_only) q.decode_schedule = schedule;
            q.batch = batch; q.h = s[0]; q.w = s[1]; q.lanes = lanes; q.rows = rows != 0; q.table_len = 64;
            q.decode = decode != 0; q.fast_image = q.decode; q.decoder_lds = q.decode ? 124 * 1024 : 0;
            q.cus = cus; q.schedule = decode_only ? BASIC_SCAN_SCHEDULE_AUTO : schedule; q.force = static_cast<ScanKernel>(force); q.lane_max_batch = gate;
            ScanLaunch L;
            ++requests;
            if (plan_scan(&g, q, &L)) { ++refused; continue; }
            bool good = true;
            if (L.kernel == ScanKernel::kNone) {
                ++per_step;
                good = gate >= 0;
            } else {
                ++planned;
                good = L.launches >= 1 && L.images >= 1 && L.launches == (batch + L.images - 1) / L.images && L.grid >= 1 && L.grid <= cus &&
                       L.lds_bytes >= kMinLds && L.lds_bytes <= kMaxLds;
                // a band decode launch: its grid holds the decoder wavefronts of its images' slots (one per slot and lane, four to a
                // workgroup), and the raster schedule never gets there
                if (q.decode && L.kernel == ScanKernel::kBand)
                    good = good && q.rows && L.images <= band_images_per_launch(&g, q.h, q.w, cus) &&
                           L.grid == compute_workgroups(&g, L.kernel, L.images, q.h, q.w) + (L.images * std::min(band_slots(&g, q.w), q.h) * lanes + 3) / 4;
                if (q.decode && q.rows && q.force == ScanKernel::kNone && q.decode_schedule == BASIC_SCAN_SCHEDULE_RASTER)
                    good = good && L.kernel != ScanKernel::kBand && L.kernel != ScanKernel::kWavefront;
            }
            if (!good && ++violations <= 20)
                printf("VIOLATION geometry %d (C %d k %d) cus %d call %dx%dx%d decode %d schedule %d force %d lane_max_batch %d lanes %d rows %d -> kernel %d launches %d "
                       "images %d grid %d lds %zu\n", geometries, g.C, g.ksize, cus, batch, s[0], s[1], decode, schedule, force, gate, lanes, rows,
                       static_cast<int>(L.kernel), L.launches, L.images, L.grid, L.lds_bytes);
        }
    }
    printf("geometries %d requests %ld planned %ld refused %ld per-step %ld violations %ld\n", geometries, requests, planned, refused, per_step, violations);
    return violations || !geometries ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "replay")) return replay();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep(false);
    if (argc == 2 && !strcmp(argv[1], "sweep-decode")) return sweep(true);
    fprintf(stderr, "usage: scan_plan_check replay|sweep|sweep-decode < lines (see the comment at the top of scan_plan_check.cpp)\n");
    return 2;
}
