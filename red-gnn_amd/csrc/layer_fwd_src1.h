// Single-source walk of the layer forward (walk code 8; layer_fwd_src1.hip): hop 0 of a query batch, enumerated from the subjects.
#pragma once
#include "common.h"

namespace rgsrc1 {

struct Src1Args {
  int B, W;
  const int32_t* sub;         // [B] the queries' subjects (rg_frontier.sub; -1 = none)
  const int32_t* out_ptr;     // rows of the out-list by tail
  const int32_t* in_ptr;
  const uint32_t* list_pk;    // out_bt_pk, or nullptr: list_rt
  const int2* list_rt;        // out_bt_rt
  const int32_t* list_pos;    // out_bt_pos
  const int2* bm_new;         // level 1
  const float4* hidden;       // [B][ld4]: row b = the state of (b, subject)
  const float4* rela;
  int ld4;
  const float4* a_s;          // [B][ap4]
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  float4* agg;
};

// one workgroup row per query; `max_out_deg` sizes the second grid dimension (the chunks of a hub subject's list are spread over it)
int launch(const Src1Args& A, int ld4, int ap4, int max_out_deg, hipStream_t s);

}  // namespace rgsrc1
