// Stand-alone host program: slide_plan / band_plan (unmicst_amd/csrc/umx_pipeline.hip) on a handful of the cases of
// tests/test_pipeline_plan_cpu.py, for a sanitizer run of the schedules outside Python.  No device is used.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/pipeline_plan_main.hip unmicst_amd/csrc/umx_pipeline.hip -o /tmp/pipeline_plan_main && /tmp/pipeline_plan_main
// It prints each plan's lines and exits 0; a plan that breaks one of the checks below, or a sanitizer report, is a failure.
#include "../unmicst_amd/csrc/umx_internal.h"

using namespace umx;

static umx_hparams hp_of(int graph, int imSize, int nChannels, int nClasses, int nOut0, int nLayers, int ks, int nExtra) {
    return umx_hparams{graph, imSize, nChannels, nClasses, nOut0, nLayers, ks, nExtra, 2};
}

// every image row up once, every tile once, every output row stitched and sent down once; event indices inside the plan's count
static int run_slide(const char* what, const umx_hparams& hp, int H, int W, const SlideSpec& sp) {
    const TileGeom g = geom_of(hp, H, W);
    const SlidePlan p = slide_plan(g, sp);
    printf("-- %s: %d x %d, groups of %d\n%s", what, H, W, sp.max_batch, slide_describe(p).c_str());
    int up = 0, tiles = 0, st = 0, dn = 0, bad = 0;
    for (const Step& s : p.steps) {
        if (s.kind == kStepUpload) { bad += s.a != up || s.c >= p.nev; up = s.b; }
        if (s.kind == kStepTiles) { bad += s.a != tiles || s.b - s.a > sp.max_batch; tiles = s.b; }
        if (s.kind == kStepStitch) { bad += s.a != st; st = s.b; }
        if (s.kind == kStepDownload) { bad += s.a != dn || s.b != st; dn = s.b; }
        if (s.kind == kStepWaitUpload || s.kind == kStepDownloadEvent || s.kind == kStepFlag) bad += s.a < 0 || s.a >= p.nev;
    }
    bad += up != H || tiles != g.npr * g.npc || st != H || dn != H;
    return bad ? 1 : 0;
}

// the launch groups hold the band's tiles once; the slabs of every rank end where its rows end
static int run_band(const char* what, const umx_hparams& hp, int H, int W, BandSpec sp) {
    const TileGeom g = geom_of(hp, H, W);
    int pa, pb, r0, r1;
    umx_geom::band(g.npr, sp.world, sp.rank, &pa, &pb);
    umx_geom::needed(pa, pb, g.sub, g.margin, g.P, H, &r0, &r1);
    sp.band_row0 = r0;
    sp.band_rows = r1 - r0;
    const BandPlan p = band_plan(g, sp);
    printf("-- %s: rank %d of %d, %d x %d, %d slab(s), groups of %d\n%s", what, sp.rank, sp.world, H, W, sp.nslabs, sp.max_batch, band_describe(p).c_str());
    long long tiles = 0;
    int bad = 0;
    for (const BandPlan::Group& G : p.groups) {
        tiles += G.t1 - G.t0;
        bad += G.t0 < pa * g.npc || G.t1 > pb * g.npc || G.ev >= p.nev;
        bad += G.r1 > G.r0 && (G.r0 < r0 || G.r1 > r1);
    }
    bad += tiles != (long long)(pb - pa) * g.npc || (int)p.slabs.size() != p.n || p.slabs.back().g1 != (int)p.groups.size();
    for (int q = 0; q < sp.world; ++q) {
        int y0, y1;
        umx_geom::owned(p.A[q], p.B[q], g.npr, g.sub, g.margin, H, &y0, &y1);
        bad += p.slabs[0].ra[q] != y0 || std::max(p.slabs[0].ra[q], p.slabs.back().rb[q]) != y1;
    }
    return bad ? 1 : 0;
}

int main() {
    const umx_hparams duo = hp_of(UMX_GRAPH_V2, 32, 2, 3, 12, 3, 3, 0), legacy = hp_of(UMX_GRAPH_LEGACY, 32, 1, 3, 8, 2, 5, 1);
    const umx_hparams big = hp_of(UMX_GRAPH_V2, 256, 2, 3, 36, 5, 3, 0), solo = hp_of(UMX_GRAPH_V2, 64, 1, 3, 80, 4, 3, 0);
    int bad = 0;
    SlideSpec sp;
    sp.max_batch = 2; sp.K = 3; sp.C_img = 2; sp.tile_flops = 1e8;
    bad += run_slide("float64 planes, several slabs", duo, 70, 45, sp);
    sp.src_bits = 16; sp.rescale = 1; sp.out_u8 = 1; sp.raw_gather = true;
    bad += run_slide("raw planes, range found by the host", duo, 113, 61, sp);
    sp.sync_call = false;
    bad += run_slide("submitted: range reduced on the device", duo, 113, 61, sp);
    sp.raw_gather = false; sp.has_range = true;
    bad += run_slide("range handed in, rows converted slab by slab", duo, 31, 200, sp);
    sp.max_batch = 32; sp.C_img = 1; sp.src_bits = 8; sp.has_range = false; sp.sync_call = true;
    bad += run_slide("one launch group: one stream", legacy, 5, 7, sp);
    sp.max_batch = 256; sp.C_img = 2; sp.src_bits = 16; sp.sync_call = false; sp.raw_gather = true; sp.tile_flops = 2e10;
    bad += run_slide("the metric slide's width, 2048 rows", big, 2048, 16384, sp);
    for (int rank = 0; rank < 3; ++rank) {
        BandSpec b;
        b.world = 3; b.rank = rank; b.nslabs = 2; b.max_batch = 8; b.K = 3;
        bad += run_band("device band", duo, 181, 77, b);
        b.staged = true; b.own_stream = rank != 1; b.gather_el = 1;
        bad += run_band("staged host band", duo, 181, 77, b);
    }
    BandSpec b;
    b.world = 8; b.rank = 5; b.nslabs = 4; b.max_batch = 256; b.K = 3; b.staged = true; b.own_stream = true; b.gather_el = 1;
    bad += run_band("a world larger than the patch rows", duo, 25, 77, b);
    b.rank = 1;
    bad += run_band("a world larger than the patch rows", duo, 25, 77, b);
    b.world = 2; b.rank = 0;
    bad += run_band("16384 rows of 64-pixel tiles", solo, 16384, 77, b);
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
