// Host program of tests/test_plan_fusion_select.py: the plan-level selectors of csrc/conv_select.hip (conv_gap_select, scale_add_select)
// over a file of vse_op records, one line per pair they accept.  The selectors read the records alone, so nothing here touches a GPU;
// the kernel families are stubs (no selector looks into a family's table).
//   usage: plan_select_host OPS.bin      (the bytes of an ir.OP_DT array)
//   gap <i> bm <row tile> tiles <per image> slots <read by the finish pass> atomic <0|1> off <workspace offset of the partials>
//           moved <0|1: they are not in the pool's scratch view>
//   scale_add <i> residual <in0|in1>
#include "../video-subtitle-extractor_amd/csrc/conv_select.hip"

#include <vector>

static ConvFamily no_family() { return ConvFamily{nullptr, nullptr, 0}; }
ConvFamily conv_gemm_family() { return no_family(); }
ConvFamily conv_smallm_family() { return no_family(); }
ConvFamily conv_mfma_family() { return no_family(); }
ConvFamily conv_patch_family() { return no_family(); }
ConvFamily conv_col_family() { return no_family(); }
ConvFamily conv_c3_family() { return no_family(); }
ConvFamily conv_pw_family() { return no_family(); }
ConvFamily conv_dwpw_family() { return no_family(); }
ConvFamily conv_head_family() { return no_family(); }
ConvFamily conv_stem_family() { return no_family(); }
ConvFamily conv_c3pool_family() { return no_family(); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<vse_op> ops;
    vse_op o;
    while (fread(&o, sizeof o, 1, f) == 1) ops.push_back(o);
    fclose(f);
    const int n = (int)ops.size();
    int levels = 0;
    for (const vse_op& q : ops) levels = std::max(levels, std::max(q.p[P_WLIN], q.p[P_WLOUT]));
    for (int i = 0; i + 1 < n; ++i) {
        // (vse_plan_create asks conv_gap_select for plans without width levels only)
        const ConvGap g = levels ? ConvGap{0, 0, 0, 0, 0, 0, 0} : conv_gap_select(ops.data(), n, i);
        if (g.fused)
            printf("gap %d bm %d tiles %d slots %d atomic %d off %lld moved %d\n", i, g.bm, g.tiles_img, g.slots, g.atomic, (long long)g.part_off,
                   g.part_off != ops[i + 1].in2.off);
        const int sa = scale_add_select(ops.data(), n, i);
        if (sa) printf("scale_add %d residual %s\n", i, sa == 1 ? "in1" : "in0");
    }
    return 0;
}
