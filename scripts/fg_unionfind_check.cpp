// Host check of csrc/volume_fg_unionfind.h (--foreground): the three passes of mud_volume_fg_label, run by one
// thread in forward, backward and shuffled voxel order with the header's own fg_find / fg_union, against a breadth-first labelling,
// on the adversarial masks of tests/test_volume_foreground_gpu.py.  It also checks parent[i] <= i after every pass.  No GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mu-diff_amd/csrc scripts/fg_unionfind_check.cpp -o fg_check && ./fg_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "volume_fg_unionfind.h"

static const int TX = 32, TY = 8, TZ = 4;
typedef std::vector<uint8_t> Mask;

struct Shape {
  int X, Y, Z;
  int n() const { return X * Y * Z; }
  int at(int x, int y, int z) const { return (z * Y + y) * X + x; }
};

static std::vector<int> reference(const Mask& m, const Shape& s, int value) {      // breadth-first, the smallest index first
  std::vector<int> lab(s.n(), -1), queue;
  for (int i = 0; i < s.n(); ++i) {
    if ((m[i] != 0) != (value != 0) || lab[i] >= 0) continue;
    lab[i] = i;
    queue.assign(1, i);
    for (size_t h = 0; h < queue.size(); ++h) {
      const int j = queue[h], x = j % s.X, y = (j / s.X) % s.Y, z = j / (s.X * s.Y);
      const int nb[6][3] = {{x - 1, y, z}, {x + 1, y, z}, {x, y - 1, z}, {x, y + 1, z}, {x, y, z - 1}, {x, y, z + 1}};
      for (auto& c : nb) {
        if (c[0] < 0 || c[0] >= s.X || c[1] < 0 || c[1] >= s.Y || c[2] < 0 || c[2] >= s.Z) continue;
        const int k = s.at(c[0], c[1], c[2]);
        if ((m[k] != 0) == (value != 0) && lab[k] < 0) lab[k] = i, queue.push_back(k);
      }
    }
  }
  return lab;
}

static bool invariant(const std::vector<int>& parent, const char* when) {
  for (int i = 0; i < (int)parent.size(); ++i)
    if (parent[i] > i || parent[i] < -1) {
      std::printf("  parent[%d] = %d breaks parent[i] <= i %s\n", i, parent[i], when);
      return false;
    }
  return true;
}

// the three passes; `order` says in which order the voxels (of a tile, then of the volume) take their turn
static bool labelled(const Mask& m, const Shape& s, int value, const std::vector<int>& want, std::mt19937* shuffle, bool backward) {
  const bool on = value != 0;
  std::vector<int> labels(s.n(), -7);
  auto ordered = [&](int count) {
    std::vector<int> o(count);
    std::iota(o.begin(), o.end(), 0);
    if (backward) std::reverse(o.begin(), o.end());
    if (shuffle) std::shuffle(o.begin(), o.end(), *shuffle);
    return o;
  };
  for (int z0 = 0; z0 < s.Z; z0 += TZ)
    for (int y0 = 0; y0 < s.Y; y0 += TY)
      for (int x0 = 0; x0 < s.X; x0 += TX) {                                      // pass 1
        std::vector<int> parent(TX * TY * TZ);
        for (int l = 0; l < TX * TY * TZ; ++l) {
          const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
          parent[l] = (x < s.X && y < s.Y && z < s.Z && (m[s.at(x, y, z)] != 0) == on) ? l : -1;
        }
        for (int l : ordered(TX * TY * TZ)) {
          if (parent[l] < 0) continue;
          const int lx = l % TX, ly = (l / TX) % TY, lz = l / (TX * TY);
          if (lx > 0 && parent[l - 1] >= 0) fg_union<fg_host_memory>(parent.data(), l, l - 1);
          if (ly > 0 && parent[l - TX] >= 0) fg_union<fg_host_memory>(parent.data(), l, l - TX);
          if (lz > 0 && parent[l - TX * TY] >= 0) fg_union<fg_host_memory>(parent.data(), l, l - TX * TY);
        }
        if (!invariant(parent, "in a tile")) return false;
        for (int l = 0; l < TX * TY * TZ; ++l) {
          const int x = x0 + l % TX, y = y0 + (l / TX) % TY, z = z0 + l / (TX * TY);
          if (x >= s.X || y >= s.Y || z >= s.Z) continue;
          int label = -1;
          if (parent[l] >= 0) {
            const int r = fg_find<fg_host_memory>(parent.data(), l);
            label = s.at(x0 + r % TX, y0 + (r / TX) % TY, z0 + r / (TX * TY));
          }
          labels[s.at(x, y, z)] = label;
        }
      }
  if (!invariant(labels, "after pass 1")) return false;
  for (int i : ordered(s.n())) {                                                  // pass 2
    const int x = i % s.X, y = (i / s.X) % s.Y, z = i / (s.X * s.Y);
    if ((m[i] != 0) != on) continue;
    if (x > 0 && x % TX == 0 && (m[i - 1] != 0) == on) fg_union<fg_host_memory>(labels.data(), i, i - 1);
    if (y > 0 && y % TY == 0 && (m[i - s.X] != 0) == on) fg_union<fg_host_memory>(labels.data(), i, i - s.X);
    if (z > 0 && z % TZ == 0 && (m[i - s.X * s.Y] != 0) == on) fg_union<fg_host_memory>(labels.data(), i, i - s.X * s.Y);
  }
  if (!invariant(labels, "after pass 2")) return false;
  for (int i : ordered(s.n())) {                                                  // pass 3
    const int p = labels[i];
    if (p < 0 || p == i) continue;
    labels[i] = fg_find<fg_host_memory>(labels.data(), p);
  }
  if (!invariant(labels, "after pass 3")) return false;
  for (int i = 0; i < s.n(); ++i)
    if (labels[i] != want[i]) {
      std::printf("  voxel %d: label %d, expected %d\n", i, labels[i], want[i]);
      return false;
    }
  return true;
}

static Mask serpentine(const Shape& s) {       // one voxel wide, through every second row of every second plane: one component
  Mask m(s.n(), 0);
  int x = 0, y = 0, dirx = 1, diry = 1;
  for (int z = 0; z < s.Z; z += 2) {
    for (;;) {                                   // snake over the rows y, y +- 2, ... of this plane
      for (;;) {
        m[s.at(x, y, z)] = 1;
        if (x + dirx < 0 || x + dirx >= s.X) break;
        x += dirx;
      }
      dirx = -dirx;
      if (y + 2 * diry < 0 || y + 2 * diry >= s.Y) break;
      m[s.at(x, y + diry, z)] = 1;
      y += 2 * diry;
    }
    diry = -diry;
    if (z + 2 < s.Z) m[s.at(x, y, z + 1)] = 1;
  }
  return m;
}

int main() {
  const Shape shapes[] = {{37, 29, 23}, {5, 4, 3}, {70, 19, 11}, {1, 1, 1}, {33, 9, 5}};
  std::mt19937 rng(7);
  int failures = 0, runs = 0;
  for (const Shape& s : shapes) {
    std::vector<std::pair<std::string, Mask>> masks;
    masks.push_back({"all on", Mask(s.n(), 1)});
    masks.push_back({"all off", Mask(s.n(), 0)});
    Mask one(s.n(), 0);
    one[s.n() / 2] = 1;
    masks.push_back({"single voxel", one});
    Mask checker(s.n()), comb(s.n(), 0);
    for (int z = 0; z < s.Z; ++z)
      for (int y = 0; y < s.Y; ++y)
        for (int x = 0; x < s.X; ++x) {
          checker[s.at(x, y, z)] = (x + y + z) % 2 == 0;
          comb[s.at(x, y, z)] = (x % 2 == 0 && y % 2 == 0) || z == s.Z - 1;       // teeth along z that join only in the last plane
        }
    masks.push_back({"checkerboard", checker});
    masks.push_back({"serpentine", serpentine(s)});
    masks.push_back({"comb", comb});
    for (double density : {0.3, 0.5, 0.7}) {
      Mask r(s.n());
      std::bernoulli_distribution coin(density);
      for (auto& v : r) v = coin(rng);
      masks.push_back({"random " + std::to_string(density), r});
    }
    for (auto& [name, m] : masks)
      for (int value : {1, 0}) {
        const std::vector<int> want = reference(m, s, value);
        if (name == "serpentine" && value == 1)
          for (int i = 0; i < s.n(); ++i)
            if (want[i] > 0) {
              std::printf("the serpentine is not one component\n");
              return 2;
            }
        for (int mode = 0; mode < 4; ++mode) {
          std::mt19937 local(100 + mode);
          const bool ok = labelled(m, s, value, want, mode >= 2 ? &local : nullptr, mode == 1);
          runs += 1;
          if (!ok) {
            failures += 1;
            std::printf("FAILED: %d x %d x %d, %s, value %d, order %d\n", s.X, s.Y, s.Z, name.c_str(), value, mode);
          }
        }
      }
  }
  std::printf("%d runs, %d failures\n", runs, failures);
  return failures ? 1 : 0;
}
