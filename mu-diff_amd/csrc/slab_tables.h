// The group tables of the slab constraints (slab.hip, slab_kspace.hip; DESIGN.md sections 5.27, 5.28): the host tables members / weights /
// gains [groups][L] packed into what one launch takes by value, every refusal made while packing, and the copy of the rows of no group.
#pragma once
#include <vector>
#include "keyed_rows.h"

#define SL_GROUPS 32             // groups per launch
#define SL_SLOTS 128             // member slots per launch (>= MUD_SLAB_MAX_MEMBERS): 32 rows of L = 5 or 16 are one launch

// the tables of one launch, passed by value like es_taps: the unused tails (-1) are squeezed out, the order is the table's
struct sl_tables {
  int start[SL_GROUPS + 1];      // group q of the launch owns slots start[q] .. start[q + 1] - 1
  int member[SL_SLOTS];          // row index
  float w[SL_SLOTS];
  float g[SL_SLOTS];
};

// members / weights / gains [groups][L] -> the launches' tables; every refusal before any launch.  owner[r] = 1 for a row in a group.
static int sl_pack(const char* who, const int32_t* members, const float* weights, const float* gains, int groups, int L, int rows,
                   std::vector<sl_tables>& launches, std::vector<int>& first_group, std::vector<int>& n_groups, std::vector<uint8_t>& owner) {
  owner.assign((size_t)rows, 0);
  sl_tables cur = {};
  int ng = 0, ns = 0;
  for (int g = 0; g < groups; ++g) {
    int cnt = 0;
    for (int l = 0; l < L; ++l) cnt += members[(size_t)g * L + l] >= 0 ? 1 : 0;
    MUD_REQUIRE(cnt > 0, "%s: members: group %d has no member", who, g);
    if (ng == SL_GROUPS || ns + cnt > SL_SLOTS) {
      cur.start[ng] = ns;
      launches.push_back(cur);
      n_groups.push_back(ng);
      ng = ns = 0;
    }
    if (ng == 0) first_group.push_back(g);
    cur.start[ng] = ns;
    for (int l = 0; l < L; ++l) {
      const int32_t m = members[(size_t)g * L + l];
      if (m == -1) continue;
      MUD_REQUIRE(m >= 0 && m < rows, "%s: members: group %d names row %d outside [0, %d)", who, g, (int)m, rows);
      MUD_REQUIRE(!owner[m], "%s: members: row %d is named twice", who, (int)m);
      owner[m] = 1;
      const float w = weights[(size_t)g * L + l];
      MUD_REQUIRE(w > 0.f && w - w == 0.f, "%s: weights: group %d, member %d is not a finite positive number", who, g, l);
      cur.member[ns] = m;
      cur.w[ns] = w;
      cur.g[ns] = 0.f;
      if (gains) {
        const float gn = gains[(size_t)g * L + l];
        MUD_REQUIRE(gn > 0.f && gn - gn == 0.f, "%s: gains: group %d, member %d is not a finite positive number", who, g, l);
        cur.g[ns] = gn;
      }
      ++ns;
    }
    ++ng;
  }
  if (ng) {
    cur.start[ng] = ns;
    launches.push_back(cur);
    n_groups.push_back(ng);
  }
  return MUD_OK;
}


// the rows of no group: x_new -> out, bit for bit, run by run
static int sl_copy_free_rows(const char* who, const float* x_new, float* out, const std::vector<uint8_t>& owner, int rows, int64_t row_len, void* stream) {
  for (int r = 0; r < rows;) {
    if (owner[r]) {
      ++r;
      continue;
    }
    int e = r;
    while (e < rows && !owner[e]) ++e;
    if (hipMemcpyAsync(out + (int64_t)r * row_len, x_new + (int64_t)r * row_len, (size_t)(e - r) * row_len * sizeof(float), hipMemcpyDeviceToDevice,
                       (hipStream_t)stream) != hipSuccess) {
      mud_set_error("%s: copying the free rows failed", who);
      return MUD_ERR_LAUNCH;
    }
    r = e;
  }
  return MUD_OK;
}
