// The row loop of the DCN head, textually shared by dcn_head_kernel (csrc/dcn.hip) and dcn_head_ordered_kernel
// (csrc/dcn_owned.hip): included INSIDE the kernel body, after its prologue, so that the default kernel compiles to
// what it compiled to before the ordered form existed (a template over a sink object moved its register allocation).
// Expects in scope: DcnHead p; lane, wave; F, H, L; grads; oDcb, oWo, oBo; and the macro DCN_HEAD_TERM(e, v), which
// receives every term of the weight gradients: e the index in [dcw: L*F | dcb: L*F | dWo: H + F | dbo], v the value.
// Wave w of workgroup g takes units 4 g + w, 4 g + w + 4 G, ... in ascending order, the pos row of a unit before its
// neg row; one lane of the wave names a given e.  Writes pred, dh, dx0 and the loss partials.
  const float* Wod = p.Wo;
  const float* Woc = p.Wo + H;
  float bw[kDcnMaxL], boc, betaL[kDcnEF];
  dcn_cross_consts(p.cw, p.cb, Woc, p.bo, L, F, lane, bw, boc, betaL);
  __syncthreads();

  float loss = 0.0f;
  const int64_t rows_per_unit = p.bpr ? 2 : 1;
  for (int64_t u = (int64_t)blockIdx.x * kWavesPerBlock + wave; u < p.units;
       u += (int64_t)gridDim.x * kWavesPerBlock) {
    float pr[2], q[2], pl[2][kDcnMaxL], sl[2][kDcnMaxL], al[2][kDcnMaxL + 1];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      pr[k] = q[k] = 0.0f;
      if (k < rows_per_unit) {
        const int64_t r = u + k * p.units;
        const float* x = p.x0 + r * p.ldx;
        const float* hr = p.h + r * p.ldh;
        float xv[kDcnEF];
        float tq = 0.0f, th = 0.0f;
#pragma unroll
        for (int j = 0; j < kDcnEF; ++j) {
          const int e = lane + kWave * j;
          xv[j] = e < F ? x[e] : 0.0f;
          if (e < F) tq += xv[j] * Woc[e];
        }
#pragma unroll
        for (int j = 0; j < kDcnEH; ++j) {
          const int e = lane + kWave * j;
          if (e < H) th += hr[e] * Wod[e];
        }
        float alpha = 1.0f;
#pragma unroll
        for (int l = 0; l < kDcnMaxL; ++l) {
          al[k][l] = alpha;
          pl[k][l] = sl[k][l] = 0.0f;
          if (l < L) {
            float t = 0.0f;
#pragma unroll
            for (int j = 0; j < kDcnEF; ++j) {
              const int e = lane + kWave * j;
              if (e < F) t += xv[j] * p.cw[l * F + e];
            }
            pl[k][l] = wave_sum(t);
            sl[k][l] = alpha * pl[k][l] + bw[l];
            alpha += sl[k][l];
          }
        }
        al[k][kDcnMaxL] = alpha;
        q[k] = wave_sum(tq);
        const float z = wave_sum(th) + alpha * q[k] + boc;
        pr[k] = sigmoidf(z);
        if (p.pred && lane == 0) p.pred[r] = pr[k];
      }
    }
    float dpred[2] = {0.0f, 0.0f};
    if (p.bpr) {
      const float d = pr[0] - pr[1];
      loss += softplus_neg(d);
      dpred[0] = -sigmoid_neg(d) * p.inv_batch;
      dpred[1] = -dpred[0];
    } else if (p.gpred) {
      dpred[0] = p.gpred[u];
    }
    if (!grads) continue;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < rows_per_unit) {
        const int64_t r = u + k * p.units;
        const float dz = dpred[k] * pr[k] * (1.0f - pr[k]);
        const float* hr = p.h + r * p.ldh;
        float* dhr = p.dh + r * p.lddh;
#pragma unroll
        for (int j = 0; j < kDcnEH; ++j) {
          const int e = lane + kWave * j;
          if (e < H) {
            const float hv = hr[e];
            dhr[e] = hv > 0.0f ? dz * Wod[e] : 0.0f;
            DCN_HEAD_TERM(oWo + e, dz * hv);
          }
        }
        if (lane == 0) DCN_HEAD_TERM(oBo, dz);
        const float alphaL = al[k][kDcnMaxL];
        float c[kDcnMaxL];
        float S = dz * q[k];
#pragma unroll
        for (int l = kDcnMaxL - 1; l >= 0; --l) {
          c[l] = 0.0f;
          if (l < L) {
            c[l] = S;
            S += c[l] * pl[k][l];
          }
        }
        const float* x = p.x0 + r * p.ldx;
        float xv[kDcnEF], G[kDcnEF], dx[kDcnEF];
#pragma unroll
        for (int j = 0; j < kDcnEF; ++j) {
          const int e = lane + kWave * j;
          xv[j] = e < F ? x[e] : 0.0f;
          G[j] = e < F ? dz * Woc[e] : 0.0f;
          dx[j] = 0.0f;
          if (e < F) DCN_HEAD_TERM(oWo + H + e, dz * (alphaL * xv[j] + betaL[j]));
        }
#pragma unroll
        for (int l = kDcnMaxL - 1; l >= 0; --l) {
          if (l < L) {
#pragma unroll
            for (int j = 0; j < kDcnEF; ++j) {
              const int e = lane + kWave * j;
              if (e < F) {
                dx[j] += sl[k][l] * G[j];
                DCN_HEAD_TERM(oDcb + l * F + e, G[j]);
                G[j] += c[l] * p.cw[l * F + e];
              }
            }
          }
        }
        float* dxr = p.dx0 + r * p.lddx;
#pragma unroll
        for (int j = 0; j < kDcnEF; ++j) {
          const int e = lane + kWave * j;
          if (e < F) dxr[e] = dx[j] + G[j];
        }
        float bt[kDcnEF];
#pragma unroll
        for (int j = 0; j < kDcnEF; ++j) bt[j] = 0.0f;
#pragma unroll
        for (int l = 0; l < kDcnMaxL; ++l) {
          if (l < L) {
#pragma unroll
            for (int j = 0; j < kDcnEF; ++j) {
              const int e = lane + kWave * j;
              if (e < F) {
                DCN_HEAD_TERM(l * F + e, c[l] * (al[k][l] * xv[j] + bt[j]));
                bt[j] += p.cb[l * F + e];
              }
            }
          }
        }
      }
    }
  }
  if (p.loss_partials) {
    if (lane == 0) p.loss_partials[blockIdx.x * kWavesPerBlock + wave] = loss;
    if (blockIdx.x == 0)
      for (int e = gridDim.x * kWavesPerBlock + threadIdx.x; e < YR_LOSS_PARTIALS; e += kBlock) p.loss_partials[e] = 0.0f;
  }
