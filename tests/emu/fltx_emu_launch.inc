/* tests/emu/fltx_emu_launch.inc -- the emulator's launch (host threads instead of hipLaunchKernel); included by
 * launchDecode() of text_amd/csrc/fltx_api.cpp under FLTX_EMU only.  A lane engine runs the host function its entry of
 * kLaneKernels names (the same entries as the HIP build's kernels, so a key the HIP build has no kernel for fails
 * here too); the generic engine's variants are chosen as genericKernel<W> chooses its kernels.
 * In scope: d (fltx_decoder*), P (const DecodeParams&), key, lane, W, nGrid, lds (as the HIP launch). */
  const DecodeParams* pp = &P;
  if (key.fam == kWlane && d->wlMaxT > 0) { /* the front-end kernel of fltx_wlane.h: grid (rows / 4, utterances), four waves per workgroup */
    emuLaunch(pp->tokRowBlocks * nGrid, 256, 4 * sizeof(WlFrontLds), [pp](char* smem) { wlTokBeamRows(*pp, smem); });
  }
  if (lane) {
    const LaneFn fn = lane->fn;
    emuLaunch(nGrid, W, lds, [pp, fn](char* smem) { fn(*pp, smem); });
    return FLTX_OK;
  }
  const int gmax = d->lean;
  const int gt = d->lane;
  const bool hot = !d->wsInLds && d->hotBytes > 0;
  emuLaunch(nGrid, W, lds, [pp, gmax, gt, hot](char* smem) {
    char* base = pp->gws ? pp->gws + (size_t)blockIdx.x * pp->gwsStride : smem;
    if (hot) {
      if (gmax == 255) {
        decodeUtterance<255>(*pp, base, smem);
      } else {
        decodeUtterance<0>(*pp, base, smem);
      }
      return;
    }
    const bool ft = pp->Kt >= pp->N;
    if (gt == 4) {
      if (pp->logAdd) {
        ft ? decodeUtterance<1, 4, true, true>(*pp, base) : decodeUtterance<1, 4, true, false>(*pp, base);
      } else {
        ft ? decodeUtterance<1, 4, false, true>(*pp, base) : decodeUtterance<1, 4, false, false>(*pp, base);
      }
    } else if (gt == 8) {
      if (pp->logAdd) {
        ft ? decodeUtterance<1, 8, true, true>(*pp, base) : decodeUtterance<1, 8, true, false>(*pp, base);
      } else {
        ft ? decodeUtterance<1, 8, false, true>(*pp, base) : decodeUtterance<1, 8, false, false>(*pp, base);
      }
    } else if (gmax == 6) {
      decodeUtterance<6>(*pp, base);
    } else if (gmax == 12) {
      decodeUtterance<12>(*pp, base);
    } else if (gmax == 255) {
      decodeUtterance<255>(*pp, base);
    } else {
      decodeUtterance<0>(*pp, base);
    }
  });
  return FLTX_OK;
