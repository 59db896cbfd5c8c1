/* FrameEncoder::compressFrame for one picture of the encoder object (encoder_impl.h): the picture's context (reference lists, weighted copies, slice and analysis parameters),
 * the row gates of pictures coded in parallel, the in-loop filters by rows and by columns, the slice NAL unit (reference: source/encoder/frameencoder.cpp:470-1130, :880-960,
 * framefilter.cpp:559-664, reference.cpp:51-185). */
#include "encoder_impl.h"

/* what the analysis and the slice header of one picture need, derived from the picture's lists (DPB::prepareEncode has run) */
/* MotionReference with weights (reference.cpp:51-185): the weighted copy of a reference picture that the motion searches of ONE slice read (luma; chroma too when the
 * sub-sample refinement measures chroma, subme > 2), made CTU row by CTU row as the reference picture's rows become final (applyWeight).  The copy is the pointwise
 * weight_pp_c of the padded plane: the margins of the reconstruction repeat its edge samples, so weighting them is what extending the weighted rows gives. */
struct WPlane
{
    Pic* src = nullptr; x265amd_weight w[3]; pixel* buf = nullptr; bool chroma[3] = { false, false, false };
    std::mutex mu; std::vector<uint8_t> rowDone; hipStream_t st = nullptr;
    ~WPlane() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } xa_scratch_free(buf); }
};
struct FrameCtx
{
    int stype = 0;
    std::vector<uint64_t> planes;           /* reference pictures (distinct), then the weighted copies of this slice (wplanes), then the reconstruction, then the source: 3 addresses each */
    int numRefs = 0;
    std::vector<std::unique_ptr<WPlane>> wplanes;
    int32_t mePic[2][16];
    x265amd_mvpred_info info;
    x265amd_inter_search_params sp;
    x265amd_slice_info si;
    x265amd_analysis_params ap;
    const Pic* colPic = nullptr;
    bool failed = false;
};

static void frameContext(const x265amd_encoder& e, Pic& pic, FrameCtx& c)
{
    const x265amd_param& p = e.p;
    const int stype = isBType(pic.type) ? 0 : pic.type == TYPE_P ? 1 : 2;
    c.stype = stype;
    const std::vector<PicP>* lists = pic.lists;
    std::vector<Pic*> index;
    int32_t refPic[2][16];
    memset(refPic, 0, sizeof(refPic));
    if (!e.frameParallel) memset(pic.refPoc, 0, sizeof(pic.refPoc));        /* coded in parallel: set by prepare(), other pictures' tasks may be reading it */
    for (int l = 0; l < 2; l++)
        for (size_t r = 0; r < lists[l].size(); r++)
        {
            Pic* q = lists[l][r].get();
            size_t k = std::find(index.begin(), index.end(), q) - index.begin();
            if (k == index.size()) { index.push_back(q); for (int cc = 0; cc < 3; cc++) c.planes.push_back(e.planeAddr(q->finalPlanes(), cc)); }
            refPic[l][r] = (int32_t)k;
            if (!e.frameParallel) pic.refPoc[l][r] = q->poc;
        }
    c.numRefs = (int)index.size();
    memcpy(c.mePic, refPic, sizeof(c.mePic));
    if (pic.weighted)
        for (int l = 0; l < 2; l++)
            for (size_t r = 0; r < lists[l].size(); r++)
            {
                if (!pic.wp[l][r][0].present) continue;         /* MotionReference::init is given weights only when the luma weight is there (frameencoder.cpp:573-577) */
                std::unique_ptr<WPlane> wpl(new WPlane);
                wpl->src = lists[l][r].get();
                memcpy(wpl->w, pic.wp[l][r], sizeof(wpl->w));
                wpl->rowDone.assign(e.ctuH, 0);
                if (xa_scratch_alloc((void**)&wpl->buf, e.picElems * sizeof(pixel)) != hipSuccess || hipStreamCreateWithFlags(&wpl->st, hipStreamNonBlocking) != hipSuccess) { c.failed = true; return; }
                wpl->chroma[0] = true;
                for (int cc = 1; cc < 3; cc++) wpl->chroma[cc] = p.subpelRefine > 2 && pic.wp[l][r][cc].present;     /* numInterpPlanes (reference.cpp:56) */
                c.mePic[l][r] = (int32_t)(c.planes.size() / 3);
                for (int cc = 0; cc < 3; cc++) c.planes.push_back(wpl->chroma[cc] ? e.planeAddr(wpl->buf, cc) : e.planeAddr(wpl->src->finalPlanes(), cc));
                c.wplanes.push_back(std::move(wpl));
            }
    for (int cc = 0; cc < 3; cc++) c.planes.push_back(e.planeAddr(pic.dRec, cc));
    for (int cc = 0; cc < 3; cc++) c.planes.push_back(e.planeAddr(pic.dSrc, cc));

    x265amd_mvpred_info& info = c.info;
    memset(&info, 0, sizeof(info));
    info.pic_width = e.W; info.pic_height = e.H; info.is_inter_b = stype == 0; info.max_num_merge_cand = p.maxNumMergeCand;
    info.num_ref_idx[0] = (int32_t)lists[0].size(); info.num_ref_idx[1] = (int32_t)lists[1].size();
    info.temporal_mvp = p.bEnableTemporalMvp != 0; info.col_from_l0 = stype != 0; info.check_ldc = stype != 0; info.poc = pic.poc;
    memcpy(info.ref_poc, pic.refPoc, sizeof(info.ref_poc));
    c.colPic = stype == 2 ? nullptr : (stype == 1 ? lists[0][0].get() : lists[1][0].get());
    if (c.colPic) { info.col_poc = c.colPic->poc; memcpy(info.col_ref_poc, c.colPic->refPoc, sizeof(info.col_ref_poc)); }

    x265amd_inter_search_params& sp = c.sp;
    memset(&sp, 0, sizeof(sp));
    sp.search_method = p.searchMethod; sp.subpel_refine = p.subpelRefine; sp.search_range = p.searchRange; sp.qp = pic.sliceQp; sp.chroma_mc = 1;
    sp.frame_parallel = e.frameParallel;
    memcpy(sp.ref_pic, refPic, sizeof(sp.ref_pic));
    memcpy(sp.me_pic, c.mePic, sizeof(sp.me_pic));
    if (pic.weighted) { sp.weighted = stype == 1 ? 1 : 2; memcpy(sp.wp, pic.wp, sizeof(sp.wp)); }
    sp.lowres_blocks_in_row = e.lowCuW;
    for (int l = 0; l < 2; l++)
        for (size_t r = 0; r < lists[l].size(); r++)
        {
            const int diffPoc = abs(pic.poc - lists[l][r]->poc);
            const std::vector<int16_t>& f = l ? pic.lowMvs1[diffPoc < 18 ? diffPoc : 0] : pic.lowMvs[diffPoc < 18 ? diffPoc : 0];
            if (diffPoc <= p.bframes + 1 && diffPoc < 18 && !f.empty()) sp.lowres_mvs[l][r] = (uint64_t)(uintptr_t)f.data();
        }

    x265amd_slice_info& si = c.si;
    memset(&si, 0, sizeof(si));
    si.pic_width = e.W; si.pic_height = e.H; si.slice_type = stype; si.slice_qp = pic.sliceQp;
    si.num_ref_idx[0] = info.num_ref_idx[0]; si.num_ref_idx[1] = info.num_ref_idx[1];
    si.max_num_merge_cand = p.maxNumMergeCand; si.sign_hide = (p.bEnableSignHiding != 0 ? X265AMD_SLICE_SIGN_HIDE : 0) | (e.lowPassDct ? X265AMD_SLICE_LOWPASS_DCT : 0); si.wpp = p.bEnableWavefront != 0;
    si.use_dqp = e.useDqp; si.max_cu_dqp_depth = e.maxCuDqpDepth;
    si.max_cu_depth = 3; si.max_amp_depth = p.bEnableAMP ? 3 : 0; si.tu_log2_min = 2; si.tu_log2_max = 5;
    si.tu_max_depth_inter = p.tuQTMaxInterDepth; si.tu_max_depth_intra = p.tuQTMaxIntraDepth;

    x265amd_analysis_params& ap = c.ap;
    memset(&ap, 0, sizeof(ap));
    ap.psy_rd = p.psyRd; ap.rd_level = p.rdLevel; ap.early_skip = p.bEnableEarlySkip != 0; ap.rskip = p.recursionSkipMode; ap.limit_refs = p.limitReferences;
    ap.b_intra = p.bIntraInBFrames != 0; ap.rect = p.bEnableRectInter != 0; ap.amp = p.bEnableAMP != 0; ap.limit_modes = p.limitModes != 0;
    ap.strong_intra_smoothing = p.bEnableStrongIntraSmoothing != 0; ap.use_sao = e.picSao(pic);           /* per picture under --selective-sao (frameencoder.cpp:684-699 asks the slice) */
    ap.fast_intra = p.bEnableFastIntra != 0; ap.limit_tu = p.limitTU;
    ap.rdoq_level = p.rdoqLevel; ap.psy_rdoq_scale = p.rdoqLevel ? p.psyRdoqFix8 : 0;      /* encoder.cpp:3667: no psy-rdoq without RDOQ */
}

/* slice header (Entropy::codeSliceHeader inputs as DPB / Encoder set them) + the sub-streams -> the picture's NAL unit */
static int sliceNal(const x265amd_encoder& e, Pic& pic, const FrameCtx& c, const int32_t* saoFlags, const std::vector<uint8_t>& data, const std::vector<uint32_t>& sizes, int nsub)
{
    const x265amd_param& p = e.p;
    x265amd_slice_header h;
    memset(&h, 0, sizeof(h));
    h.nal_unit_type = pic.nalType; h.temporal_id_plus1 = 1; h.first_in_access_unit = 1;
    h.slice_type = c.stype; h.poc = pic.poc; h.last_idr_poc = pic.lastIDR; h.log2_max_poc_lsb = 8; h.rps_idx = -1; h.num_rps_in_sps = 0;
    h.num_negative = (int32_t)pic.neg.size(); h.num_positive = (int32_t)pic.pos.size();
    {
        int j = 0;
        for (const PicP& q : pic.neg) { h.delta_poc[j] = q->poc - pic.poc; h.used[j++] = pic.rpsUsed; }
        for (const PicP& q : pic.pos) { h.delta_poc[j] = q->poc - pic.poc; h.used[j++] = pic.rpsUsed; }
    }
    h.temporal_mvp_enabled = p.bEnableTemporalMvp != 0;
    /* a picture --selective-sao leaves out says so with two zero flags (entropy.cpp:647-658); selectiveSAO is non-zero whenever the SPS says SAO */
    h.use_sao = e.picSao(pic); h.selective_sao = e.selectiveSAO; h.sao_luma = saoFlags[0]; h.sao_chroma = saoFlags[1];
    h.num_ref_idx[0] = c.info.num_ref_idx[0]; h.num_ref_idx[1] = c.info.num_ref_idx[1]; h.num_ref_idx_default[0] = h.num_ref_idx_default[1] = 1;
    h.col_from_l0 = c.stype != 0; h.col_ref_idx = 0; h.max_num_merge_cand = p.maxNumMergeCand;
    h.slice_qp = pic.sliceQp; h.pps_init_qp = 26; h.deblocking_disabled = !p.bEnableLoopFilter;
    h.slfase_flag = (0x5f4e4a53u >> (pic.poc % 31)) & 1;                                              /* SLFASE_CONSTANT (dpb.cpp:294) */
    h.wpp = p.bEnableWavefront != 0;
    h.weighted_pred = p.bEnableWeightedPred != 0; h.weighted_bipred = p.bEnableWeightedBiPred != 0; h.luma_log2_weight_denom = pic.lumaDenom; h.chroma_log2_weight_denom = pic.chromaDenom;
    memcpy(h.wp, pic.wp, sizeof(h.wp));
    size_t dataBytes = 0;
    for (int s = 0; s < nsub; s++) dataBytes += sizes[s];
    pic.nalBytes.assign(dataBytes * 3 / 2 + 4096, 0);
    const size_t n = x265amd_write_slice_nal(&h, data.data(), sizes.data(), nsub, pic.nalBytes.data(), pic.nalBytes.size());
    if (!n || n > pic.nalBytes.size()) return xa_fail(X265AMD_EINVAL, "encoder: slice NAL");
    pic.nalBytes.resize(n);
    return 0;
}

/* --rskip 2, before the CTU loop of a P / B picture (FrameEncoder::compressFrame, frameencoder.cpp:474-484: computeEdge on the source picture at the coded size, padding
 * included): one launch of the device pass on the picture's stream, its counts written into mapped host memory kept with the picture, one wait.  What every CTU row of the
 * picture reads afterwards -- under WPP and with pictures coded in parallel alike -- is that one array. */
int x265amd_encoder::edgeCounts(Pic& pic, hipStream_t st, x265amd_rskip_edge& edge)
{
    const int bw = (W + 31) / 32, bh = (H + 31) / 32;
    if (!pic.dSrc) return xa_fail(X265AMD_EINVAL, "encoder: the picture's source is gone");
    if (!pic.edgeCounts && xa_mapped_alloc((void**)&pic.edgeCounts, (size_t)bw * bh * sizeof(uint32_t), true) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: edge counts");
    const int rc = x265amd_rskip_edge_counts(st, planeAddr(pic.dSrc, 0), stride, W, H, pic.edgeCounts);
    if (rc != X265AMD_OK) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: edge counts");
    edge.counts = pic.edgeCounts; edge.blocks_w = bw; edge.threshold = p.edgeVarThreshold;
    return X265AMD_OK;
}

/* --psnr / --ssim: what FrameFilter::processPostRow measures row by row after SAO (framefilter.cpp:667-711), as picture-wide passes over the source and the FINAL
 * reconstruction, both in device memory, once the picture's last row is final; a few words come back (x265amd_picture_ssd / _ssim, csrc/quality_kernels.hip) and
 * Encoder::finishFrameStats' values are made of them (x265amd_quality_finish).  On the picture's own stream, waited for here: the picture is handed out after its task. */
int x265amd_encoder::measureQuality(Pic& pic, hipStream_t st)
{
    if (!pic.dSrc) return xa_fail(X265AMD_EINVAL, "encoder: the picture's source is gone");
    const pixel* fin = pic.finalPlanes();
    const int nb = X265AMD_SSIM_BANDS(H);
    const size_t ssdBytes = 3 * sizeof(uint64_t), bandBytes = (size_t)nb * sizeof(x265amd_ssim_band), workBytes = X265AMD_SSIM_WORK_BYTES(W, H);
    struct Scratch { void* p = nullptr; ~Scratch() { xa_scratch_free(p); } } dev;
    if (xa_scratch_alloc(&dev.p, ssdBytes + bandBytes + workBytes) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: quality record");
    uint64_t* dSsd = (uint64_t*)dev.p;
    x265amd_ssim_band* dBands = (x265amd_ssim_band*)((char*)dev.p + ssdBytes);
    std::vector<uint64_t> host((ssdBytes + bandBytes) / sizeof(uint64_t), 0);
    if (p.bEnablePsnr)
    {
        const uint64_t srcP[3] = { planeAddr(pic.dSrc, 0), planeAddr(pic.dSrc, 1), planeAddr(pic.dSrc, 2) };
        const uint64_t recP[3] = { planeAddr(fin, 0), planeAddr(fin, 1), planeAddr(fin, 2) };
        const int rc = x265amd_picture_ssd(st, srcP, recP, stride, cstride, W, H, srcW, srcH, dSsd);
        if (rc != X265AMD_OK) return rc;
    }
    if (p.bEnableSsim)
    {
        const int rc = x265amd_picture_ssim(st, planeAddr(pic.dSrc, 0), planeAddr(fin, 0), stride, W, H, dBands, (char*)dev.p + ssdBytes + bandBytes, 0);
        if (rc != X265AMD_OK) return rc;
    }
    /* (what a switch that is off leaves unwritten is not read below) */
    if (hipMemcpyAsync(host.data(), dev.p, ssdBytes + bandBytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return xa_fail(X265AMD_EHIP, "encoder: quality passes");
    const uint64_t* ssd = p.bEnablePsnr ? host.data() : nullptr;
    const x265amd_ssim_band* bands = p.bEnableSsim ? (const x265amd_ssim_band*)(host.data() + 3) : nullptr;
    x265amd_quality_values v;
    const int rc = x265amd_quality_finish(ssd, bands, nullptr, W, H, srcW, srcH, &v);
    if (rc != X265AMD_OK) return xa_fail(rc, "encoder: quality values");
    x265amd_quality& q = pic.quality;
    if (ssd) { for (int k = 0; k < 3; k++) q.ssd[k] = ssd[k]; q.psnrY = v.psnrY; q.psnrU = v.psnrU; q.psnrV = v.psnrV; q.psnr = v.psnr; q.measured |= 1; }
    if (bands)
    {
        double sum = 0.0;       /* FrameEncoder::m_ssim: a double that takes every band's float (framefilter.cpp:708) */
        for (int r = 0; r < nb; r++) { float f; memcpy(&f, &bands[r].sum_bits, sizeof(float)); sum += f; }
        q.ssimSum = sum; q.ssimCnt = v.ssimCnt; q.ssim = v.ssim; q.measured |= 2;
    }
    return X265AMD_OK;
}

/* the buffers one picture's analysis reads and fills, and the slice data behind it (runFrame, runFrameParallel) */
struct FrameBufs
{
    std::vector<x265amd_mv_unit> noCol;                 /* all zero: the collocated field of a picture that has none */
    std::vector<uint8_t> refDepth; std::vector<int8_t> refQp0;         /* per list, of its first picture: the units' depths, CUData::m_qp[0] of the CTUs */
    std::vector<x265amd_cu_stat> stat; std::vector<int16_t> coeff; std::vector<uint8_t> data; std::vector<uint32_t> sizes; int nsub = 0;
    XaTuRecs tuRecs = { nullptr, { nullptr, nullptr } };
    x265amd_rskip_edge edge = { nullptr, 0, 0.0f };     /* (an I picture never asks: its record goes in without counts) */
    FrameBufs(const x265amd_encoder& e, const FrameCtx& fc)
        : noCol(fc.colPic ? 0 : (size_t)e.w4 * e.h4), refDepth(2 * (size_t)e.w4 * e.h4, 0), refQp0(2 * (size_t)e.nctu, 0), stat((size_t)e.nctu + 1),
          coeff((size_t)e.nctu * RD_TILE_ELEMS, 0), data((size_t)e.W * e.H * 3 + (1u << 16)), sizes((size_t)e.ctuH + 1, 0) {}
};
/* the picture as the analysis takes it (x265amd_host.h); pic.units, pic.motion and pic.tuRecs have their sizes by now */
static XaAnalysisArgs analysisArgs(const x265amd_encoder& e, Pic& pic, FrameCtx& fc, FrameBufs& b)
{
    const bool limitTU = e.p.limitTU >= 3;
    if (limitTU)
    {
        b.tuRecs.cur = pic.tuRecs.data();
        for (int l = 0; l < 2; l++) if (!pic.lists[l].empty() && pic.lists[l][0]->tuRecs.size() == pic.tuRecs.size()) b.tuRecs.ref[l] = pic.lists[l][0]->tuRecs.data();
    }
    return { e.me, &fc.info, &fc.sp, &fc.si, &fc.ap, pic.units.data(), pic.motion.data(), fc.colPic ? fc.colPic->motion.data() : b.noCol.data(), b.refDepth.data(), b.refQp0.data(),
             fc.planes.data(), (int)(fc.planes.size() / 3), e.stride, e.cstride, b.stat.data(), e.useDqp ? pic.cuQp.data() : nullptr, limitTU ? &b.tuRecs : nullptr,
             e.p.recursionSkipMode == 2 ? &b.edge : nullptr };
}

/* FrameEncoder::compressFrame for one picture (its own thread and HIP stream).  The analysis starts when every reference picture is final; the
 * in-loop filters, SAO (its decision carries state from picture to picture, SAO::m_depthSaoRate) and the shared filter scratch run in coding
 * order, i.e. after the previous picture's task. */
int x265amd_encoder::runFrame(const PicP& picp, std::shared_future<int> prev)
{
    Pic& pic = *picp;
    for (int l = 0; l < 2; l++)
        for (const PicP& q : pic.lists[l]) if (q->done.valid() && q->done.get() != 0) return X265AMD_EHIP;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: stream");
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } guard{ st };
    const std::vector<PicP>* lists = pic.lists;
    FrameCtx fc;
    frameContext(*this, pic, fc);
    if (fc.failed) return xa_fail(X265AMD_EHIP, "encoder: weighted reference planes");
    for (auto& wpl : fc.wplanes)            /* one picture at a time: the reference pictures are complete, so are their weighted copies */
        if (weightRows(*wpl, 0, ctuH - 1) != X265AMD_OK) return X265AMD_EHIP;
    x265amd_mvpred_info& info = fc.info;
    x265amd_slice_info& si = fc.si;

    const size_t nUnits = (size_t)w4 * h4;
    pic.units.assign(nUnits, x265amd_cu_unit()); pic.motion.assign(nUnits, x265amd_mv_unit());
    memset(pic.units.data(), 0, sizeof(x265amd_cu_unit) * nUnits); memset(pic.motion.data(), 0, sizeof(x265amd_mv_unit) * nUnits);
    FrameBufs bufs(*this, fc);
    for (int l = 0; l < 2; l++)
        if (!lists[l].empty())
        {
            const Pic* q = lists[l][0].get();
            for (size_t i = 0; i < nUnits; i++) bufs.refDepth[l * nUnits + i] = q->units[i].depth;
            for (int i = 0; i < nctu; i++) bufs.refQp0[(size_t)l * nctu + i] = useDqp ? q->units[(size_t)(i / ctuW) * 16 * w4 + (size_t)(i % ctuW) * 16].qp : (int8_t)q->sliceQp;      /* CUData::m_qp[0] of the co-located CTU */
        }
    const bool sao = picSao(pic);
    if (useDqp && pic.cuQp.empty()) return xa_fail(X265AMD_EINVAL, "encoder: the picture has no CU QPs");
    if (p.limitTU >= 3) pic.tuRecs.assign((size_t)nctu * 21, -1);
    if (p.recursionSkipMode == 2 && si.slice_type != 2) { const int erc = edgeCounts(pic, st, bufs.edge); if (erc != X265AMD_OK) return erc; }
    int rc = xa_analyse_frame(analysisArgs(*this, pic, fc, bufs), st, bufs.coeff.data(), nullptr, sao ? nullptr : bufs.data.data(), bufs.data.size(), bufs.sizes.data(), &bufs.nsub, nullptr);
    if (rc != X265AMD_OK) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: analysis");

    /* ---- from here on in coding order ---- */
    if (prev.valid() && prev.get() != 0) return X265AMD_EHIP;
    pixel* recY = pic.dRec + org[0]; pixel* recU = pic.dRec + org[1]; pixel* recV = pic.dRec + org[2];
    const bool saoPre = sao && saoNonDeblock;
    if (saoPre)
    {
        /* --sao-non-deblock: the statistics of every CTU's right and bottom strips while nothing is deblocked yet (SAO::calcSaoStatsCu_BeforeDblk, frameencoder.cpp:1599) */
        const uint64_t recP[3] = { planeAddr(pic.dRec, 0), planeAddr(pic.dRec, 1), planeAddr(pic.dRec, 2) };
        const uint64_t srcP[3] = { planeAddr(pic.dSrc, 0), planeAddr(pic.dSrc, 1), planeAddr(pic.dSrc, 2) };
        rc = x265amd_sao_stats_pre(st, recP, srcP, stride, cstride, W, H, dSaoPreCount, dSaoPreOrg);
        if (rc != X265AMD_OK) return rc;
    }
    if (p.bEnableLoopFilter)
    {
        std::vector<x265amd_deblock_unit> dbu(nUnits);
        rc = x265amd_deblock_units(&si, &info, pic.units.data(), pic.motion.data(), dbu.data());
        if (rc != X265AMD_OK) return rc;
        if (hipMemcpyAsync(dDbUnits, dbu.data(), sizeof(x265amd_deblock_unit) * nUnits, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return xa_fail(X265AMD_EHIP, "encoder: deblock upload");
        rc = x265amd_deblock_picture(st, recY, recU, recV, stride, cstride, W, H, dDbUnits, p.deblockingFilterBetaOffset, p.deblockingFilterTCOffset, 0, 0, 0, 3);
        if (rc != X265AMD_OK) return rc;
        if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: deblock");
    }
    int32_t saoFlags[2] = { 0, 0 };
    if (sao)
    {
        const size_t nstat = (size_t)nctu * 3 * 5 * 32;
        const uint64_t recP[3] = { planeAddr(pic.dRec, 0), planeAddr(pic.dRec, 1), planeAddr(pic.dRec, 2) };
        const uint64_t srcP[3] = { planeAddr(pic.dSrc, 0), planeAddr(pic.dSrc, 1), planeAddr(pic.dSrc, 2) };
        if (hipMemsetAsync(dSaoCount, 0, nstat * 4, st) != hipSuccess || hipMemsetAsync(dSaoOrg, 0, nstat * 4, st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: sao memset");
        const int statFlags = saoStatFlags(pic);
        rc = x265amd_sao_stats_opt(st, recP, srcP, stride, cstride, W, H, dSaoCount, dSaoOrg, statFlags);
        if (rc != X265AMD_OK) return rc;
        std::vector<int32_t> cnt(nstat), orgs(nstat), preCnt(saoPre ? nstat : 0), preOrgs(saoPre ? nstat : 0);
        if (saoPre && (hipMemcpyAsync(preCnt.data(), dSaoPreCount, nstat * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                       hipMemcpyAsync(preOrgs.data(), dSaoPreOrg, nstat * 4, hipMemcpyDeviceToHost, st) != hipSuccess))
            return xa_fail(X265AMD_EHIP, "encoder: sao download");
        if (hipMemcpyAsync(cnt.data(), dSaoCount, nstat * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(orgs.data(), dSaoOrg, nstat * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return xa_fail(X265AMD_EHIP, "encoder: sao download");
        std::vector<x265amd_sao_ctu> sparams((size_t)nctu);
        memset(sparams.data(), 0, sizeof(x265amd_sao_ctu) * nctu);
        rc = x265amd_sao_rdo_opt(&si, pic.type != TYPE_B ? 1 : 0, 1, p.qpMin, p.qpMax,       /* IS_REFERENCED: fixed by the type (hasReferences changes as later pictures are prepared) */
                                 pic.units.data(), cnt.data(), orgs.data(), depthSaoRate, sparams.data(), saoFlags,
                                 statFlags, limitSAO, saoPre ? preCnt.data() : nullptr, saoPre ? preOrgs.data() : nullptr);
        if (rc != X265AMD_OK) return rc;
        if (hipMemcpyAsync(dSaoParams, sparams.data(), sizeof(x265amd_sao_ctu) * nctu, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(dSaoTmp, pic.dRec, picElems * sizeof(pixel), hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return xa_fail(X265AMD_EHIP, "encoder: sao upload");
        const uint64_t dstP[3] = { planeAddr(dSaoTmp, 0), planeAddr(dSaoTmp, 1), planeAddr(dSaoTmp, 2) };
        rc = x265amd_sao_apply(st, recP, dstP, stride, cstride, W, H, dSaoParams);
        if (rc != X265AMD_OK) return rc;
        if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: sao");
        std::swap(pic.dRec, dSaoTmp);
        recY = pic.dRec + org[0]; recU = pic.dRec + org[1]; recV = pic.dRec + org[2];
        rc = x265amd_encode_slice_data(&si, pic.units.data(), bufs.coeff.data(), sparams.data(), saoFlags, bufs.data.data(), bufs.data.size(), bufs.sizes.data(), &bufs.nsub);
        if (rc != X265AMD_OK) return rc;
    }
    /* the reconstruction becomes a reference: extend its borders */
    rc = x265amd_extend_pic_border(st, recY, stride, W, H, marginX, marginY);
    if (rc == X265AMD_OK) rc = x265amd_extend_pic_border(st, recU, cstride, W / 2, H / 2, marginX / 2, marginY / 2);
    if (rc == X265AMD_OK) rc = x265amd_extend_pic_border(st, recV, cstride, W / 2, H / 2, marginX / 2, marginY / 2);
    if (rc != X265AMD_OK) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: border extension");
    if (p.bEnablePsnr || p.bEnableSsim) { rc = measureQuality(pic, st); if (rc != X265AMD_OK) return rc; }

    rc = sliceNal(*this, pic, fc, saoFlags, bufs.data, bufs.sizes, bufs.nsub);
    if (rc) return rc;
    /* the source is no longer needed (unless the weight analysis of later pictures reads its chroma planes: weightAnalyse works on source pictures); the reconstruction
     * stays while the picture is referenced.  The reference lists are only needed by pictures that are still to come through their own lists */
    if (!keepSources()) { xa_scratch_free(pic.dSrc); pic.dSrc = nullptr; }
    return 0;
}

/* ---- pictures coded in parallel (param.frameNumThreads > 1) ----
 * FrameEncoder::compressFrame as the reference runs it with several frame encoders (frameencoder.cpp:880-960, :1930-1960; framefilter.cpp:559-664): a CTU row
 * of this picture starts when every reference picture has finished the rows down to refLagRows below it, and the in-loop filters follow the analysis row by
 * row so that the rows of this picture become available to the pictures that reference it while its lower rows are still being analysed. */
struct RowGate { x265amd_encoder* e; Pic* pic; std::vector<Pic*> refs; std::vector<uint8_t>* refDepth; size_t nUnits; FrameCtx* fc = nullptr; std::vector<int8_t>* refQp0 = nullptr; };

/* What a CTU may read of a reference picture, and when.  The reference waits for whole rows: row + refLagRows rows of every reference picture before a row
 * starts (frameencoder.cpp:893-908).  What the row's commands can actually read is less -- vectors end searchRange samples below the block (search.cpp:92,
 * :2763; merge / AMVP candidates beyond are left out), plus sub-sample steps and interpolation taps: the rows row - 2 .. row + 2 at most -- and pictures here
 * are published by COLUMNS (Pic::finalX, filterRowsCols): a CTU starts when those rows of every reference picture are final two CTUs to its right, which covers
 * ordinary vectors, the co-located CTUs' motion and the co-located depths; every command that reads reference samples first asks gateRefReady with its exact
 * reach (xa_ref_guard_*), so a long vector waits for exactly what it needs.  A picture therefore follows its reference pictures a few CTUs behind instead of
 * rows behind, and the slow last CTU row of a picture (cut CTUs when the height is no multiple of 64) no longer holds up every picture behind it.  Results do
 * not depend on any of this: a sample is only ever read when it is final.  (Deadlock freedom with few device queues: a row takes its queue when it starts, and
 * it starts only when finalX of the rows it will follow is above zero, i.e. when those rows hold their queues and run.) */
/* the per-CTU gate: the rows row - 2 .. row + 1 of every reference picture final up to 56 samples beyond the CTU to the right (vectors up to that length, the
 * co-located CTUs' motion and depths), row + 2 begun (a vector reaching into its first lines is rare: gateRefWait then waits for it, and the row holds its queue) */
static inline int gateNeed(const x265amd_encoder& e, int col) { return std::min(e.W, 64 * col + 120); }
static int gateCtuReady(void* ctx, int row, int col)        /* polled (the start condition of a row task): 1 yes, 0 not yet, -1 a reference picture failed */
{
    RowGate& g = *(RowGate*)ctx;
    const x265amd_encoder& e = *g.e;
    const int need = gateNeed(e, col), r0 = std::max(0, row - 2), r1 = std::min(e.ctuH - 1, row + 1);
    for (Pic* q : g.refs)
    {
        if (q->failed.load(std::memory_order_acquire)) return -1;
        if (row + 2 < e.ctuH && q->published(row + 2) < 1) return 0;
        for (int r = r1; r >= r0; r--) if (q->published(r) < need) return 0;
    }
    return 1;
}
static int gateRowReady(void* ctx, int row) { return gateCtuReady(ctx, row, 0); }
static int gateCtuWait(void* ctx, int row, int col)         /* blocking: the task parks on the counters */
{
    RowGate& g = *(RowGate*)ctx;
    const x265amd_encoder& e = *g.e;
    const int need = gateNeed(e, col), r0 = std::max(0, row - 2), r1 = std::min(e.ctuH - 1, row + 1);
    static const bool pubLog = xa_env_present("X265AMD_PUB_LOG");
    for (Pic* q : g.refs)
        for (int r = r1; r >= r0; r--)
        {
            if (q->published(r) < need)
            {
                const double t0 = pubLog ? Pic::pubClockMs() : 0;
                xa_wait_counter(q->finalX[r], (uint64_t)need);
                if (pubLog) fprintf(stderr, "x265amd gate: poc %d row %d col %d waited from %.2f to %.2f for poc %d row %d x %d\n", g.pic->poc, row, col, t0, Pic::pubClockMs(), q->poc, r, need);
            }
            if (q->failed.load(std::memory_order_acquire)) return -1;
        }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}
static int gateRefWait(void* ctx, int picIdx, int yMin, int yMax, int xMax)
{
    RowGate& g = *(RowGate*)ctx;
    const x265amd_encoder& e = *g.e;
    if (picIdx >= (int)g.refs.size() && g.fc && picIdx - (int)g.refs.size() < (int)g.fc->wplanes.size())
    {
        /* a weighted copy (a motion search of a slice with weights): whole CTU rows of the reference picture, then the copy's rows (MotionReference::applyWeight at the
         * row's start, frameencoder.cpp:900-908) */
        WPlane& wpl = *g.fc->wplanes[picIdx - (int)g.refs.size()];
        Pic* q = wpl.src;
        const int r0 = std::min(std::max(yMin, 0), e.H - 1) >> 6, r1 = std::min(std::max(yMax, 0), e.H - 1) >> 6;
        const int wc = xa_task_wait_class(3);
        for (int r = r1; r >= r0; r--)
        {
            if (q->published(r) < e.W) xa_wait_counter(q->finalX[r], (uint64_t)e.W);
            if (q->failed.load(std::memory_order_acquire)) { xa_task_wait_class(wc); return -1; }
        }
        xa_task_wait_class(wc);
        std::atomic_thread_fence(std::memory_order_acquire);
        return g.e->weightRows(wpl, r0, r1) == X265AMD_OK ? 0 : -1;
    }
    if (picIdx < 0 || picIdx >= (int)g.refs.size()) return 0;          /* the picture itself / the source: not a reference */
    Pic* q = g.refs[picIdx];
    const int need = xMax >= e.W - 1 ? e.W : std::max(0, xMax + 1);
    const int r0 = std::min(std::max(yMin, 0), e.H - 1) >> 6, r1 = std::min(std::max(yMax, 0), e.H - 1) >> 6;
    const int wc = xa_task_wait_class(3);
    for (int r = r1; r >= r0; r--)
    {
        if (q->published(r) < need) xa_wait_counter(q->finalX[r], (uint64_t)need);
        if (q->failed.load(std::memory_order_acquire)) { xa_task_wait_class(wc); return -1; }
    }
    xa_task_wait_class(wc);
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}
/* what gateCtuWait(row, col) has waited for (XaRowHooks::ctu_reach) */
static void gateCtuReach(void* ctx, int row, int col, int* r0, int* r1, int* need)
{
    const x265amd_encoder& e = *((RowGate*)ctx)->e;
    *need = gateNeed(e, col); *r0 = std::max(0, row - 2); *r1 = std::min(e.ctuH - 1, row + 1);
}
static void gateBeforeRow(void*, int) {}
static void gateBeforeCtu(void* ctx, int row, int col)
{
    RowGate& g = *(RowGate*)ctx;
    const x265amd_encoder& e = *g.e;
    /* the co-located CTU's depths (topSkipMinDepth reads refFrameList[l][0] at this CTU's address): that CTU of the reference picture is coded now */
    for (int l = 0; l < 2; l++)
        if (!g.pic->lists[l].empty())
        {
            const Pic* q = g.pic->lists[l][0].get();
            const int y0 = row * 16, y1 = std::min(e.h4, y0 + 16), x0 = col * 16, x1 = std::min(e.w4, x0 + 16);
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) (*g.refDepth)[l * g.nUnits + (size_t)y * e.w4 + x] = q->units[(size_t)y * e.w4 + x].depth;
            /* ... and its first unit's QP (topSkipMinDepth's previousQP: CUData::m_qp[0] of that CTU as it was coded) */
            if (e.useDqp && g.refQp0) (*g.refQp0)[(size_t)l * e.nctu + (size_t)row * e.ctuW + col] = q->units[(size_t)y0 * e.w4 + x0].qp;
        }
}
static void gateAfterCtu(void* ctx, int row, int col)
{
    RowGate& g = *(RowGate*)ctx;
    { std::lock_guard<std::mutex> lk(g.pic->mu); g.pic->analysedCols[row] = col + 1; }
    g.pic->cv.notify_all();
}
static void gateAfterRow(void* ctx, int row)
{
    RowGate& g = *(RowGate*)ctx;
    { std::lock_guard<std::mutex> lk(g.pic->mu); g.pic->analysedRows = row + 1; }
    g.pic->cv.notify_all();
}

/* CTU rows r0 .. r1 of a weighted copy (MotionReference::applyWeight, reference.cpp:118-185): weight_pp_c over the rows' padded lines -- with the first row the top margin, with
 * the last the bottom margin -- of the planes that carry a weight.  The rows of the reference picture are final (the caller has waited for them). */
int x265amd_encoder::weightRows(WPlane& wpl, int r0, int r1)
{
    std::lock_guard<std::mutex> lk(wpl.mu);
    bool any = false;
    xa_thread_device();
    for (int r = r0; r <= r1; r++)
    {
        if (r < 0 || r >= ctuH || wpl.rowDone[r]) continue;
        for (int cc = 0; cc < 3; cc++)
        {
            if (!wpl.chroma[cc]) continue;
            const int sh = cc ? 1 : 0, h = H >> sh, my = marginY >> sh, mx = marginX >> sh, rows = 64 >> sh;
            const intptr_t st = cc ? cstride : stride;
            const int y0 = r == 0 ? -my : rows * r, y1 = r == ctuH - 1 ? h + my : rows * (r + 1);
            const intptr_t at = (intptr_t)org[cc] + (intptr_t)y0 * st - mx;
            const x265amd_weight& w = wpl.w[cc];
            const int correction = 14 - X265AMD_DEPTH;
            const int rc = x265amd_weight_buffer(wpl.st, wpl.src->finalPlanes() + at, wpl.buf + at, (size_t)(y1 - y0) * st, w.w, (w.denom ? 1 << (w.denom - 1) : 0) << correction,
                                                 w.denom + correction, w.o * (1 << (X265AMD_DEPTH - 8)));
            if (rc != X265AMD_OK) return rc;
        }
        any = true;
    }
    if (any && hipStreamSynchronize(wpl.st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: weighted reference rows");
    for (int r = std::max(r0, 0); r <= r1 && r < ctuH; r++) wpl.rowDone[r] = 1;
    return X265AMD_OK;
}

/* The filter thread of a picture: FrameFilter::processRow / processPostRow for each CTU row as the analysis delivers it.  Row r is deblocked when row r + 1
 * is analysed (its vertical edges, then its horizontal edges, which reach three samples up into row r - 1); its SAO statistics follow (they leave out the samples
 * the rows below still change) and its parameters are decided; row r - 1 can then be offset (its last lines and the line below them are final), its borders
 * extended and the row published.  The last row publishes itself. */
int x265amd_encoder::filterRows(Pic& pic, const x265amd_slice_info& si, const x265amd_mvpred_info& info, std::vector<x265amd_sao_ctu>& sparams, int32_t* saoFlags)
{
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: stream");
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } guard{ st };
    const bool sao = picSao(pic), dbl = p.bEnableLoopFilter != 0, saoPre = sao && saoNonDeblock;
    const int statFlags = saoStatFlags(pic);
    const size_t nUnits = (size_t)w4 * h4, nstat = (size_t)nctu * 3 * 5 * 32, rowStat = (size_t)ctuW * 3 * 5 * 32;
    struct Scratch { void* p = nullptr; ~Scratch() { xa_scratch_free(p); } } dDb, dCnt, dOrg, dPar, dPreCnt, dPreOrg;
    std::vector<x265amd_deblock_unit> dbu;
    std::vector<int32_t> cnt, orgs, preCnt, preOrgs;
    int preRows = 0;            /* --sao-non-deblock: CTU rows whose pre-deblock statistics are enqueued */
    if (dbl) { if (xa_scratch_alloc(&dDb.p, sizeof(x265amd_deblock_unit) * nUnits) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: device allocation"); dbu.resize(nUnits); }
    if (sao)
    {
        if (xa_scratch_alloc(&dCnt.p, nstat * 4) != hipSuccess || xa_scratch_alloc(&dOrg.p, nstat * 4) != hipSuccess || xa_scratch_alloc(&dPar.p, sizeof(x265amd_sao_ctu) * nctu) != hipSuccess)
            return xa_fail(X265AMD_EHIP, "encoder: device allocation");
        cnt.resize(nstat); orgs.resize(nstat);
        if (saoPre)
        {
            if (xa_scratch_alloc(&dPreCnt.p, nstat * 4) != hipSuccess || xa_scratch_alloc(&dPreOrg.p, nstat * 4) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: device allocation");
            preCnt.resize(nstat); preOrgs.resize(nstat);
        }
        saoFlags[0] = saoFlags[1] = 1;          /* SAO::startSlice: never switched off when pictures are coded in parallel (sao.cpp:264) */
    }
    pixel* recY = pic.dRec + org[0]; pixel* recU = pic.dRec + org[1]; pixel* recV = pic.dRec + org[2];
    const uint64_t recP[3] = { planeAddr(pic.dRec, 0), planeAddr(pic.dRec, 1), planeAddr(pic.dRec, 2) };
    const uint64_t srcP[3] = { planeAddr(pic.dSrc, 0), planeAddr(pic.dSrc, 1), planeAddr(pic.dSrc, 2) };
    pixel* fin = sao ? pic.dFin : pic.dRec;
    const uint64_t finP[3] = { planeAddr(fin, 0), planeAddr(fin, 1), planeAddr(fin, 2) };
    double unusedRate[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    int rc = X265AMD_OK;
    /* offsets, borders, publication of CTU row k */
    auto finish = [&](int k) -> int {
        const int y0 = k * 64, y1 = std::min(H, y0 + 64);
        if (sao)
        {
            int r = x265amd_sao_apply_rows(st, recP, finP, stride, cstride, W, H, (const x265amd_sao_ctu*)dPar.p, k, k + 1);
            if (r != X265AMD_OK) return r;
        }
        int r = x265amd_extend_border_rows(st, fin + org[0], stride, W, H, marginX, marginY, y0, y1);
        if (r == X265AMD_OK) r = x265amd_extend_border_rows(st, fin + org[1], cstride, W / 2, H / 2, marginX / 2, marginY / 2, y0 / 2, y1 / 2);
        if (r == X265AMD_OK) r = x265amd_extend_border_rows(st, fin + org[2], cstride, W / 2, H / 2, marginX / 2, marginY / 2, y0 / 2, y1 / 2);
        if (r != X265AMD_OK) return r;
        if (hipStreamSynchronize(st) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: row filters");
        pic.publish(k, W);
        return X265AMD_OK;
    };
    static const bool timing = xa_env_present("X265AMD_TIMING");
    double tPh[6] = { 0, 0, 0, 0, 0, 0 };
    auto tLast = std::chrono::steady_clock::now();
    auto stamp = [&](int k) { if (!timing) return; const auto n = std::chrono::steady_clock::now(); tPh[k] += std::chrono::duration<double, std::milli>(n - tLast).count(); tLast = n; };
    struct Report { const bool& on; double* t; int poc; ~Report() { if (on) fprintf(stderr, "x265amd: filter rows of poc %d (ms): waiting %.1f, deblock units + upload %.1f, deblock %.1f, sao statistics %.1f, sao decision + upload %.1f, offsets + borders %.1f\n", poc, t[0], t[1], t[2], t[3], t[4], t[5]); } } report{ timing, tPh, pic.poc };
    for (int r = 0; r < ctuH && rc == X265AMD_OK; r++)
    {
        stamp(5);
        {
            std::unique_lock<std::mutex> lk(pic.mu);
            /* intra prediction of row r + 1 reads the unfiltered last line of row r: FrameEncoder::m_filterRowDelay (frameencoder.cpp:124-126, :1936-1950) */
            const int needRows = (dbl || sao) ? std::min(ctuH, r + 2) : r + 1;
            pic.cv.wait(lk, [&] { return pic.analysedRows >= needRows || pic.failed; });
            if (pic.failed) return X265AMD_EHIP;
        }
        stamp(0);
        const int y4b = r * 16, y4e = std::min(h4, y4b + 16);
        if (saoPre && preRows <= std::min(r + 1, ctuH - 1))
        {
            /* --sao-non-deblock: the pre-deblock statistics of every analysed row that has not had them (rows <= r + 1 are analysed), on this stream in front of the
             * deblocking of row r -- whose vertical edges change row r's last line, which the statistics of row r + 1 read, and whose top edge reaches up into row r - 1;
             * they read their own rows and the last line of the row above, none of it deblocked yet.  Every word of the rows' records is stored: nothing to clear */
            const int upTo = std::min(r + 1, ctuH - 1) + 1;
            rc = x265amd_sao_stats_pre_rows(st, recP, srcP, stride, cstride, W, H, (int32_t*)dPreCnt.p, (int32_t*)dPreOrg.p, preRows, upTo);
            if (rc != X265AMD_OK) break;
            preRows = upTo;
        }
        if (dbl)
        {
            rc = x265amd_deblock_units_rows(&si, &info, pic.units.data(), pic.motion.data(), dbu.data(), y4b, y4e);
            if (rc != X265AMD_OK) break;
            if (hipMemcpyAsync((x265amd_deblock_unit*)dDb.p + (size_t)y4b * w4, dbu.data() + (size_t)y4b * w4, sizeof(x265amd_deblock_unit) * (size_t)(y4e - y4b) * w4, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
            { rc = xa_fail(X265AMD_EHIP, "encoder: deblock upload"); break; }
            stamp(1);
            rc = x265amd_deblock_rows(st, recY, recU, recV, stride, cstride, W, H, (const x265amd_deblock_unit*)dDb.p, p.deblockingFilterBetaOffset, p.deblockingFilterTCOffset, 0, 0, 0, 3, y4b, y4e);
            if (rc != X265AMD_OK) break;
        }
        if (sao)
        {
            if (hipMemsetAsync((int32_t*)dCnt.p + r * rowStat, 0, rowStat * 4, st) != hipSuccess || hipMemsetAsync((int32_t*)dOrg.p + r * rowStat, 0, rowStat * 4, st) != hipSuccess)
            { rc = xa_fail(X265AMD_EHIP, "encoder: sao memset"); break; }
            rc = x265amd_sao_stats_opt_rows(st, recP, srcP, stride, cstride, W, H, (int32_t*)dCnt.p, (int32_t*)dOrg.p, statFlags, r, r + 1);
            if (rc != X265AMD_OK) break;
            if (saoPre && (hipMemcpyAsync(preCnt.data() + r * rowStat, (int32_t*)dPreCnt.p + r * rowStat, rowStat * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                           hipMemcpyAsync(preOrgs.data() + r * rowStat, (int32_t*)dPreOrg.p + r * rowStat, rowStat * 4, hipMemcpyDeviceToHost, st) != hipSuccess))
            { rc = xa_fail(X265AMD_EHIP, "encoder: sao download"); break; }
            if (hipMemcpyAsync(cnt.data() + r * rowStat, (int32_t*)dCnt.p + r * rowStat, rowStat * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipMemcpyAsync(orgs.data() + r * rowStat, (int32_t*)dOrg.p + r * rowStat, rowStat * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            { rc = xa_fail(X265AMD_EHIP, "encoder: sao download"); break; }
            stamp(3);
            int32_t flags[2] = { 1, 1 };
            rc = x265amd_sao_rdo_rows_opt(&si, pic.type != TYPE_B ? 1 : 0, 2, p.qpMin, p.qpMax, pic.units.data(), cnt.data(), orgs.data(), unusedRate, sparams.data(), flags, r, r + 1,
                                          statFlags, limitSAO, saoPre ? preCnt.data() : nullptr, saoPre ? preOrgs.data() : nullptr);
            if (rc != X265AMD_OK) break;
            if (hipMemcpyAsync((x265amd_sao_ctu*)dPar.p + (size_t)r * ctuW, sparams.data() + (size_t)r * ctuW, sizeof(x265amd_sao_ctu) * ctuW, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
            { rc = xa_fail(X265AMD_EHIP, "encoder: sao upload"); break; }
            stamp(4);
        }
        if (!dbl && !sao) { rc = finish(r); continue; }         /* nothing below changes this row */
        if (r > 0) rc = finish(r - 1);
        if (rc == X265AMD_OK && r == ctuH - 1) rc = finish(r);
    }
    return rc;
}

/* Waiting for a stream without burning a core: hipStreamSynchronize polls flat out, and the filter threads of twenty pictures in flight did that beside the worker
 * threads -- past the CPU quota of the box (16 cores), where the kernel then freezes every thread of the process for the rest of its 100 ms period (cgroup cpu.stat:
 * nr_throttled; a dozen milliseconds each time, in the middle of the encode).  An event, a short poll for the common case (the work is a few kernels), then naps. */
static hipError_t streamWaitPolite(hipStream_t st, hipEvent_t ev)
{
    const int spinUs = 30;
    if (!ev) return hipStreamSynchronize(st);
    hipError_t e = hipEventRecord(ev, st);
    if (e != hipSuccess) return e;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;)
    {
        e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(spinUs)) { for (int k = 0; k < 16; k++) __builtin_ia32_pause(); continue; }
        struct timespec ts = { 0, 20000 }; nanosleep(&ts, nullptr);
        /* a filter stream that stands for seconds: say so once (the kernels behind the event are a few microseconds each) */
        static std::atomic<int> said{ 0 };
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(3) && said.fetch_add(1) < 4)
            fprintf(stderr, "x265amd: a filter stream has not reached its event for 3 s (stream %p, hipStreamQuery says %s)\n", (void*)st, hipGetErrorName(hipStreamQuery(st)));
    }
}

/* The filter thread of a picture, by columns.  A UNIT is a CTU row r and a range of its CTU columns [c0, c1): the deblocking of the unit's edges (vertical edges
 * right of c0's left boundary up to and including c1's left boundary, then the horizontal edges of the columns, the top one reaching three samples into row
 * r - 1), the SAO statistics and decisions of its CTUs; behind it row r - 1 (and the last row itself) is offset, its borders extended and its columns published
 * up to eight samples short of the unit's right end (the offsets of those need the next unit's horizontal edges).  A unit is ready when
 *   - row r is analysed through CTU c1 (the vertical edge at its right boundary reads both sides' coding data),
 *   - row r + 1 is analysed through CTU c1 (its intra prediction has then read everything it needs of row r's last line UNFILTERED:
 *     FrameEncoder::m_filterRowDelay, frameencoder.cpp:124-126, :1936-1950),
 *   - the units of row r - 1 cover the columns (their vertical edges precede this unit's top horizontal edge, their decisions are the merge-up candidates).
 * The same samples as FrameFilter's row order produce (framefilter.cpp:559-664): vertical edges lie eight samples apart and touch three on either side, so
 * their order is free; a horizontal edge reads its own columns behind the vertical edges on both sides; a CTU's statistics leave out what the CTUs to its right
 * and below still change (sao.cpp:760-776); an offset sample is written when it and its neighbours are final.  Units are taken as large as the analysis
 * allows (a row the filter falls behind on is caught up in one unit), at least `minChunk` CTUs. */
int x265amd_encoder::filterRowsCols(Pic& pic, const x265amd_slice_info& si, const x265amd_mvpred_info& info, std::vector<x265amd_sao_ctu>& sparams, int32_t* saoFlags)
{
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: stream");
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } guard{ st };
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    struct EventGuard { hipEvent_t e; ~EventGuard() { if (e) (void)hipEventDestroy(e); } } evGuard{ ev };
    const bool sao = picSao(pic), dbl = p.bEnableLoopFilter != 0;
    const int statFlags = saoStatFlags(pic);            /* (never X265AMD_SAO_NON_DEBLOCK here: those pictures take filterRows) */
    const size_t nUnits = (size_t)w4 * h4, ctuStat = (size_t)3 * 5 * 32, nstat = (size_t)nctu * ctuStat;
    /* deblocking records, SAO statistics and parameters: mapped memory the device reads / writes in place (no staging copies, no synchronisation to free a
     * staging buffer): the records as the host derives them, the statistics as the kernel stores them, the parameters as decided. */
    XaMapped hDb, hPar; XaMappedOut hCnt, hOrg;
    if (dbl && hDb.alloc(sizeof(x265amd_deblock_unit) * nUnits) != hipSuccess)
        return xa_fail(X265AMD_EHIP, "encoder: device allocation");
    if (sao)
    {
        if (hPar.alloc(sizeof(x265amd_sao_ctu) * nctu) != hipSuccess || hCnt.alloc(nstat * 4) != hipSuccess || hOrg.alloc(nstat * 4) != hipSuccess)
            return xa_fail(X265AMD_EHIP, "encoder: device allocation");
        saoFlags[0] = saoFlags[1] = 1;          /* SAO::startSlice: never switched off when pictures are coded in parallel (sao.cpp:264) */
    }
    x265amd_deblock_unit* dbu = (x265amd_deblock_unit*)hDb.p;
    int32_t* cnt = (int32_t*)hCnt.p; int32_t* orgs = (int32_t*)hOrg.p;
    pixel* recY = pic.dRec + org[0]; pixel* recU = pic.dRec + org[1]; pixel* recV = pic.dRec + org[2];
    const uint64_t recP[3] = { planeAddr(pic.dRec, 0), planeAddr(pic.dRec, 1), planeAddr(pic.dRec, 2) };
    const uint64_t srcP[3] = { planeAddr(pic.dSrc, 0), planeAddr(pic.dSrc, 1), planeAddr(pic.dSrc, 2) };
    pixel* fin = sao ? pic.dFin : pic.dRec;
    const uint64_t finP[3] = { planeAddr(fin, 0), planeAddr(fin, 1), planeAddr(fin, 2) };
    static const bool timing = xa_env_present("X265AMD_TIMING");
    double tWait = 0, tWork = 0; int numUnits = 0, numSweeps = 0;
    auto tLast = std::chrono::steady_clock::now();
    auto lap = [&](double& acc) { if (!timing) return; const auto n = std::chrono::steady_clock::now(); acc += std::chrono::duration<double, std::milli>(n - tLast).count(); tLast = n; };
    struct Report { const bool& on; double& w; double& k; int& n; int& sw; int poc; ~Report() { if (on) fprintf(stderr, "x265amd: filter units of poc %d: %d units in %d sweeps, %.1f ms waiting for the analysis, %.1f ms filtering\n", poc, n, sw, w, k); } } report{ timing, tWait, tWork, numUnits, numSweeps, pic.poc };
    /* a picture nobody references is waited for by nobody: whole rows */
    const int minChunk = pic.type == TYPE_B ? ctuW : 2;
    /* the last rows are where a chain of pictures waits for each other (they finish last, and cut CTUs make the last row the slowest): every CTU of them at once */
    const int minChunkLast = pic.type != TYPE_B ? 1 : minChunk;
    /* which chunks a snapshot of the analysis allows, in which order, and what is final behind them: x265amd_filter_plan (host/filter_plan.cpp) */
    std::vector<int32_t> doneTop((size_t)ctuH, 0), doneFull((size_t)ctuH, 0), pubX((size_t)ctuH, 0), a((size_t)ctuH, 0);
    std::vector<uint8_t> carry((size_t)ctuH * (X265AMD_CTX_STRIDE + 8), 0);
    std::vector<x265amd_filter_step> steps((size_t)2 * ctuH);
    std::vector<x265amd_filter_finish> finish((size_t)ctuH);
    int rc = X265AMD_OK;
    /* offsets and borders of a finish range (enqueued; published behind the sweep's synchronisation) */
    auto finishCols = [&](const x265amd_filter_finish& f) -> int {
        if (sao)
        {
            int r = x265amd_sao_apply_rows_cols(st, recP, finP, stride, cstride, W, H, (const x265amd_sao_ctu*)hPar.p, f.row, f.row + 1, f.x_begin, f.x_end);
            if (r != X265AMD_OK) return r;
        }
        return xa_extend_border_band_420(st, fin + org[0], fin + org[1], fin + org[2], stride, cstride, W, H, marginX, marginY, f.y_begin, f.y_end, f.x_begin, f.x_end, f.x_begin == 0, f.x_end == W);
    };
    /* A CTU row's unit in two steps (round 4).  TOP: the vertical edges of the row's first eight lines and its top horizontal edge -- which completes the deblocking of
     * the row ABOVE -- as soon as the row itself is analysed (nothing of this touches the row's last line, which the row below still reads unfiltered); the row above can
     * then be offset, extended and published: one CTU row earlier than when everything waited for the row below.  FULL: the other vertical edges, the inner horizontal
     * edges, the statistics and the decisions, when the row below is analysed (FrameEncoder::m_filterRowDelay).  Vertical edges are decided per four lines and touch only
     * their own lines, the top horizontal edge touches lines 0-2: the samples are those of the reference's order. */
    const int earlyTop = 1;
    for (;;)
    {
        {
            std::unique_lock<std::mutex> lk(pic.mu);
            /* something to do? (a snapshot of the analysis: the rows only advance) */
            auto ready = [&]() -> bool {
                return pic.failed || x265amd_filter_ready(W, H, pic.analysedCols.data(), doneTop.data(), doneFull.data(), minChunk, minChunkLast, earlyTop) != 0;
            };
            pic.cv.wait(lk, ready);
            if (pic.failed) return X265AMD_EHIP;
            a = pic.analysedCols;
        }
        lap(tWait);
        /* ---- one sweep: every step that is ready, top row first (the stream orders them: FULL of row r - 1, TOP of row r, FULL of row r).  First the edges and the
         * statistics of all of them, one synchronisation, then the decisions on the host, then offsets + borders, a second synchronisation, then the publication:
         * two waits per sweep however many rows are in flight. ---- */
        bool all = true;
        for (int r = 0; r < ctuH; r++) if (doneFull[r] != ctuW) all = false;
        int numSteps = 0, numFinish = 0;
        if (x265amd_filter_plan(W, H, a.data(), doneTop.data(), doneFull.data(), pubX.data(), minChunk, minChunkLast, earlyTop, steps.data(), &numSteps, finish.data(), &numFinish) != X265AMD_OK)
        { rc = xa_fail(X265AMD_EINVAL, "encoder: filter plan"); break; }
        bool anyFull = false;
        for (int i = 0; i < numSteps && rc == X265AMD_OK; i++)
        {
            const x265amd_filter_step& s = steps[i];
            if (s.kind == X265AMD_FILTER_TOP)
            {
                if (!dbl) continue;
                /* the edge records of the whole row height (both steps read them) where the kernels read them: mapped memory, no copy */
                rc = x265amd_deblock_units_rect(&si, &info, pic.units.data(), pic.motion.data(), dbu, s.y4_begin, s.rec_y4_end, s.rec_x4_begin, s.rec_x4_end);
                if (rc != X265AMD_OK) break;
                _mm_sfence();       /* the records went through the write-combining BAR mapping: out of this core's buffers before the launch that reads them */
                rc = x265amd_deblock_rows_cols(st, recY, recU, recV, stride, cstride, W, H, dbu, p.deblockingFilterBetaOffset, p.deblockingFilterTCOffset, 0, 0, 0, 3, s.y4_begin, s.y4_end, s.col_begin, s.col_end);
                if (rc != X265AMD_OK) break;
            }
            else
            {
                anyFull = true;
                if (dbl && s.y4_end > s.y4_begin)
                {
                    rc = x265amd_deblock_rows_cols(st, recY, recU, recV, stride, cstride, W, H, dbu, p.deblockingFilterBetaOffset, p.deblockingFilterTCOffset, 0, 0, 0, 3, s.y4_begin, s.y4_end, s.col_begin, s.col_end);
                    if (rc != X265AMD_OK) break;
                }
                if (sao)
                {
                    /* every workgroup stores all 160 sums and counts of its (CTU, plane): nothing to clear; the host reads them where the kernel leaves them */
                    rc = x265amd_sao_stats_opt_rows_cols(st, recP, srcP, stride, cstride, W, H, cnt, orgs, statFlags, s.row, s.row + 1, s.col_begin, s.col_end);
                    if (rc != X265AMD_OK) break;
                }
            }
        }
        if (rc != X265AMD_OK) break;
        if (numSteps == 0) { if (all) break; continue; }
        numUnits += numSteps; numSweeps++;
        if (sao && anyFull)
        {
            if (streamWaitPolite(st, ev) != hipSuccess) { rc = xa_fail(X265AMD_EHIP, "encoder: sao statistics"); break; }
            for (int i = 0; i < numSteps; i++)
            {
                const x265amd_filter_step& u = steps[i];
                if (u.kind != X265AMD_FILTER_FULL) continue;
                int32_t flags[2] = { 1, 1 };
                rc = x265amd_sao_rdo_cols_opt(&si, pic.type != TYPE_B ? 1 : 0, 2, p.qpMin, p.qpMax, pic.units.data(), cnt, orgs, sparams.data(), flags, u.row, u.col_begin, u.col_end,
                                              carry.data() + (size_t)u.row * (X265AMD_CTX_STRIDE + 8), statFlags, limitSAO, nullptr, nullptr);
                if (rc != X265AMD_OK) break;
                const size_t off = (size_t)u.row * ctuW + u.col_begin, n = (size_t)(u.col_end - u.col_begin);
                memcpy((x265amd_sao_ctu*)hPar.p + off, sparams.data() + off, sizeof(x265amd_sao_ctu) * n);
                _mm_sfence();               /* as for the deblocking records above */
            }
            if (rc != X265AMD_OK) break;
        }
        /* final now: the row above a TOP step (its parameters were decided by its own FULL step, in this sweep at the latest), and the last row behind its FULL step */
        for (int i = 0; i < numFinish && rc == X265AMD_OK; i++) rc = finishCols(finish[i]);
        if (rc != X265AMD_OK) break;
        if (streamWaitPolite(st, ev) != hipSuccess) { rc = xa_fail(X265AMD_EHIP, "encoder: row filters"); break; }
        for (int i = 0; i < numFinish; i++) pic.publish(finish[i].row, finish[i].x_end);
        lap(tWork);
    }
    return rc;
}

static uint64_t thread_cpu_ns()
{
    struct timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
int x265amd_encoder::runFrameParallel(const PicP& picp)
{
    Pic& pic = *picp;
    /* whatever happens, the pictures waiting for rows of this one are released */
    struct Release { Pic& pic; int* rc; ~Release() { if (*rc) pic.fail(); } };
    int rc = X265AMD_EHIP;
    Release release{ pic, &rc };
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return xa_fail(X265AMD_EHIP, "encoder: stream");
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } guard{ st };
    const std::vector<PicP>* lists = pic.lists;
    FrameCtx fc;
    frameContext(*this, pic, fc);
    if (fc.failed) return xa_fail(X265AMD_EHIP, "encoder: weighted reference planes");
    FrameBufs bufs(*this, fc);
    RowGate gate{ this, &pic, {}, &bufs.refDepth, (size_t)w4 * h4, &fc, &bufs.refQp0 };
    if (useDqp && pic.cuQp.empty()) return xa_fail(X265AMD_EINVAL, "encoder: the picture has no CU QPs");
    for (int l = 0; l < 2; l++)
    {
        for (const PicP& q : lists[l]) if (std::find(gate.refs.begin(), gate.refs.end(), q.get()) == gate.refs.end()) gate.refs.push_back(q.get());
        if (!lists[l].empty()) for (int i = 0; i < nctu; i++) bufs.refQp0[(size_t)l * nctu + i] = (int8_t)lists[l][0]->sliceQp;
    }
    const bool sao = picSao(pic);
    std::vector<x265amd_sao_ctu> sparams((size_t)nctu);
    memset(sparams.data(), 0, sizeof(x265amd_sao_ctu) * nctu);
    int32_t saoFlags[2] = { 0, 0 };
    int filterRc = X265AMD_OK;
    /* by columns when there is something to filter and the rows run as a wavefront; the row-by-row form otherwise */
    static const bool colsOff = !xa_env_on("X265AMD_FILTER_COLS");
    /* (a picture that gathers pre-deblock statistics, --sao-non-deblock, goes by rows: the pass is not fitted into the column sweeps) */
    const bool byCols = !colsOff && p.bEnableWavefront && (p.bEnableLoopFilter || sao) && ctuH > 1 && ctuW > 1 && !(sao && saoNonDeblock);
    std::thread filters([&, byCols] { xa_thread_device(); filterRc = byCols ? filterRowsCols(pic, fc.si, fc.info, sparams, saoFlags) : filterRows(pic, fc.si, fc.info, sparams, saoFlags); if (filterRc) pic.fail();
                                      cpuFilterNs += thread_cpu_ns(); });
    /* the rows' priority among the row tasks of all pictures in flight: the picture's place in coding order */
    const uint64_t rowOrder = pic.codingOrder + 1;
    const XaRowHooks hooks{ &gate, gateRowReady, gateBeforeRow, gateAfterRow, gateCtuWait, gateBeforeCtu, gateAfterCtu, gateRefWait, rowOrder, gateCtuReach };
    /* (--limit-tu 3 / 4: the records were sized when the picture was prepared: pictures coded beside this one read them CTU by CTU behind the gate) */
    if (p.recursionSkipMode == 2 && fc.si.slice_type != 2) { const int erc = edgeCounts(pic, st, bufs.edge); if (erc != X265AMD_OK) { pic.fail(); filters.join(); return rc = erc; } }
    int arc = xa_analyse_frame(analysisArgs(*this, pic, fc, bufs), st, bufs.coeff.data(), nullptr, sao ? nullptr : bufs.data.data(), bufs.data.size(), bufs.sizes.data(), &bufs.nsub, &hooks);
    if (arc != X265AMD_OK) pic.fail();
    filters.join();
    if (arc != X265AMD_OK) return rc = arc;
    if (filterRc != X265AMD_OK) return rc = filterRc;
    /* every row is final (the filter thread's last publication; it runs with both filters off, too) and the source is still there */
    if (p.bEnablePsnr || p.bEnableSsim) { arc = measureQuality(pic, st); if (arc != X265AMD_OK) return rc = arc; }
    if (sao)
    {
        arc = x265amd_encode_slice_data(&fc.si, pic.units.data(), bufs.coeff.data(), sparams.data(), saoFlags, bufs.data.data(), bufs.data.size(), bufs.sizes.data(), &bufs.nsub);
        if (arc != X265AMD_OK) return rc = arc;
    }
    arc = sliceNal(*this, pic, fc, saoFlags, bufs.data, bufs.sizes, bufs.nsub);
    if (arc) return rc = arc;
    if (!keepSources()) { xa_scratch_free(pic.dSrc); pic.dSrc = nullptr; }
    return rc = 0;
}

