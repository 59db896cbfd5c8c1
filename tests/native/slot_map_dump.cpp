/* Prints, as JSON, every slot of the EncoderPrimitives-shaped table that x265amd_setup_primitives() is meant to fill (x265-amod_amd/csrc/table_setup.hip), from the
 * slot arithmetic of x265-amod_amd/host/primitive_table.h: slot index, kind (pu / cu / misc / chroma_pu / chroma_cu), size index, field name and variant (the
 * [NONALIGNED] / [ALIGNED] twin, or the intra mode).  Host only.  Its output is committed as tests/golden/primitive_slots.json; tests/test_primitive_table_slots.py
 * builds this program again and requires the same text, and calls every listed slot of the installed table on the GPU.
 *
 *   g++ -std=c++17 -I x265-amod_amd/host tests/native/slot_map_dump.cpp -o slot_map_dump && ./slot_map_dump > tests/golden/primitive_slots.json
 */
#include <stdio.h>
#include "primitive_table.h"

using namespace x265amd;

enum { CSP420 = 1 };
static const int k_puW[NUM_PU_SIZES] = { 4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 12, 16, 4, 32, 24, 32, 8, 64, 48, 64, 16 };
static const int k_puH[NUM_PU_SIZES] = { 4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 12, 16, 4, 16, 24, 32, 8, 32, 48, 64, 16, 64 };

static int g_count = 0;

/* variant: 0 none, 1 the two alignment twins (index al), 2 an intra mode (index al) */
static void emit(int slot, const char* kind, int size, const char* field, int variantKind = 0, int al = 0)
{
    printf("%s {\"slot\": %d, \"kind\": \"%s\", \"size\": %d, \"field\": \"%s\", \"variant\": ", g_count++ ? ",\n" : "", slot, kind, size, field);
    if (variantKind == 1) printf("\"%s\"}", al == ALIGNED ? "aligned" : "nonaligned");
    else if (variantKind == 2) printf("%d}", al);
    else printf("null}");
}

int main()
{
    printf("[\n");
    for (int i = 0; i < NUM_PU_SIZES; i++)
    {
        static const struct { int f; const char* name; } one[] = {
            { PU_sad, "sad" }, { PU_sad_x3, "sad_x3" }, { PU_sad_x4, "sad_x4" }, { PU_satd, "satd" },
            { PU_luma_hpp, "luma_hpp" }, { PU_luma_hps, "luma_hps" }, { PU_luma_vpp, "luma_vpp" }, { PU_luma_vps, "luma_vps" },
            { PU_luma_vsp, "luma_vsp" }, { PU_luma_vss, "luma_vss" }, { PU_luma_hvpp, "luma_hvpp" } };
        for (const auto& e : one) emit(slotPU(i, e.f), "pu", i, e.name);
        for (int al = 0; al < 2; al++)
        {
            emit(slotPU(i, PU_pixelavg_pp + al), "pu", i, "pixelavg_pp", 1, al);
            emit(slotPU(i, PU_addAvg + al), "pu", i, "addAvg", 1, al);
            emit(slotPU(i, PU_convert_p2s + al), "pu", i, "convert_p2s", 1, al);
        }
    }
    for (int i = 0; i < NUM_CU_SIZES; i++)
    {
        if (i < 4)      /* TU sizes 4..32 */
        {
            emit(slotCU(i, CU_dct), "cu", i, "dct"); emit(slotCU(i, CU_idct), "cu", i, "idct"); emit(slotCU(i, CU_standard_dct), "cu", i, "standard_dct");
            emit(slotCU(i, CU_copy_cnt), "cu", i, "copy_cnt"); emit(slotCU(i, CU_count_nonzero), "cu", i, "count_nonzero");
            emit(slotCU(i, CU_cpy2Dto1D_shl), "cu", i, "cpy2Dto1D_shl"); emit(slotCU(i, CU_cpy2Dto1D_shr), "cu", i, "cpy2Dto1D_shr");
            for (int al = 0; al < 2; al++) emit(slotCU(i, CU_cpy1Dto2D_shl + al), "cu", i, "cpy1Dto2D_shl", 1, al);
            emit(slotCU(i, CU_cpy1Dto2D_shr), "cu", i, "cpy1Dto2D_shr");
            emit(slotCU(i, CU_intra_pred_allangs), "cu", i, "intra_pred_allangs"); emit(slotCU(i, CU_intra_filter), "cu", i, "intra_filter");
            for (int m = 0; m < INTRA_MODES; m++) emit(slotCU(i, CU_intra_pred + m), "cu", i, "intra_pred", 2, m);
        }
        emit(slotCU(i, CU_sub_ps), "cu", i, "sub_ps");
        for (int al = 0; al < 2; al++) emit(slotCU(i, CU_add_ps + al), "cu", i, "add_ps", 1, al);
        emit(slotCU(i, CU_var), "cu", i, "var"); emit(slotCU(i, CU_sse_pp), "cu", i, "sse_pp"); emit(slotCU(i, CU_sse_ss), "cu", i, "sse_ss");
        emit(slotCU(i, CU_psy_cost_pp), "cu", i, "psy_cost_pp");
        for (int al = 0; al < 2; al++) emit(slotCU(i, CU_ssd_s + al), "cu", i, "ssd_s", 1, al);
        emit(slotCU(i, CU_sa8d), "cu", i, "sa8d"); emit(slotCU(i, CU_transpose), "cu", i, "transpose");
    }
    emit(slotMisc(M_dst4x4), "misc", 0, "dst4x4"); emit(slotMisc(M_idst4x4), "misc", 0, "idst4x4");
    emit(slotMisc(M_quant), "misc", 0, "quant"); emit(slotMisc(M_nquant), "misc", 0, "nquant");
    emit(slotMisc(M_dequant_scaling), "misc", 0, "dequant_scaling"); emit(slotMisc(M_dequant_normal), "misc", 0, "dequant_normal");
    for (int al = 0; al < 2; al++) emit(slotMisc(M_scale1D_128to64 + al), "misc", 0, "scale1D_128to64", 1, al);
    emit(slotMisc(M_scale2D_64to32), "misc", 0, "scale2D_64to32");
    emit(slotMisc(M_weight_sp), "misc", 0, "weight_sp"); emit(slotMisc(M_weight_pp), "misc", 0, "weight_pp");
    /* 4:2:0 chroma, indexed by the LUMA partition / CU: no entries of half a 4x4 partition except addAvg, satd only where the half is a multiple of 4x4 */
    for (int i = 0; i < NUM_PU_SIZES; i++)
    {
        if ((((k_puW[i] >> 1) | (k_puH[i] >> 1)) & 3) == 0) emit(slotChromaPU(CSP420, i, CPU_satd), "chroma_pu", i, "satd");
        if (i != 0)
        {
            emit(slotChromaPU(CSP420, i, CPU_filter_vpp), "chroma_pu", i, "filter_vpp"); emit(slotChromaPU(CSP420, i, CPU_filter_vps), "chroma_pu", i, "filter_vps");
            emit(slotChromaPU(CSP420, i, CPU_filter_vsp), "chroma_pu", i, "filter_vsp"); emit(slotChromaPU(CSP420, i, CPU_filter_vss), "chroma_pu", i, "filter_vss");
            emit(slotChromaPU(CSP420, i, CPU_filter_hpp), "chroma_pu", i, "filter_hpp"); emit(slotChromaPU(CSP420, i, CPU_filter_hps), "chroma_pu", i, "filter_hps");
        }
        for (int al = 0; al < 2; al++)
        {
            emit(slotChromaPU(CSP420, i, CPU_addAvg + al), "chroma_pu", i, "addAvg", 1, al);
            if (i != 0) emit(slotChromaPU(CSP420, i, CPU_p2s + al), "chroma_pu", i, "p2s", 1, al);
        }
    }
    for (int i = 1; i < NUM_CU_SIZES; i++) emit(slotChromaCU(CSP420, i, CCU_sa8d), "chroma_cu", i, "sa8d");
    printf("\n]\n");
    return 0;
}
