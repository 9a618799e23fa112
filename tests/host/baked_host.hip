// The host program of the baked marcher (tests/test_walks_host_cpu.py builds and runs it; tests/host/walk_host_build.py has the recipe).
// It includes csrc/baked.hip unchanged and calls only its __host__ __device__ functions and the host function that makes the
// lattice: no HIP call, no launch, no device.  Usage: baked_host DIR.  Every file is raw little-endian, read into a heap buffer
// of exactly the file's size (an overread lands in a redzone of a sanitizer build):
//   dims.bin    int32 [5]   Cx, Cy, Cz, R, n_bricks
//   params.bin  fp32  [9]   lo[3], hi[3], step, background, stop
//   points{0,1,2}.bin       the dense points of the degree: [Cz+1][Cy+1][Cx+1] x 16 << degree bytes
//   pool{0,1,2}.bin         the brick pool of the degree: [n_bricks][9][9][9] x 16 << degree bytes
//   slots.bin   int32 [Bz][By][Bx]        words.bin  uint32 [fine words + brick words]        rays.bin  fp32 [R][8]
// Written, with c = (degree * 2 + layout) * 2 + use_bits (layout 0 dense, 1 sparse):
//   march.bin   fp32  [12][R][5]   baked_march: rgb, depth, opacity
//   K.bin       int32 [R]          the sample count of the ray (0: a miss)
//   flags.bin   uint8 [sum K]      brute force, every k in [0, K): 1 inside the box, 2 brick bit set, 4 cell bit set, 8 slot >= 0
//   brute.bin   int32 [12][R]      the samples brute force counts before the ray ends (`stop`; with stop == 0 all that count)
//   count.bin   int32 [12][R]      the samples baked_walk handed to `visit`
//   visit.bin   int32 [sum count]  their indices, in the order of count.bin
// The index of a visited sample is found from its t: t_k does not decrease with k, so it is the first k after the last visited
// one whose t_k is the sample's (where consecutive t_k are equal the samples are the same sample, and only their number counts).
#include "baked.hip"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <thread>
#include <vector>

namespace {

struct Blob {
  void* p = nullptr;
  size_t n = 0;
};

Blob read_exact(const std::string& path, size_t want) {
  Blob b;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "baked_host: cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  b.n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  if (b.n != want) {
    fprintf(stderr, "baked_host: %s has %zu bytes, not %zu\n", path.c_str(), b.n, want);
    exit(2);
  }
  if (posix_memalign(&b.p, 64, b.n ? b.n : 1) != 0 || (b.n && fread(b.p, 1, b.n, f) != b.n)) {
    fprintf(stderr, "baked_host: cannot read %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
  return b;
}

void write_all(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, 1, n, f) != n) || fclose(f) != 0) {
    fprintf(stderr, "baked_host: cannot write %s\n", path.c_str());
    exit(2);
  }
}

struct Scene {
  BakedGrid G;
  OccDims dm;
  const uint32_t* words;
  const int32_t* slots;
  const float* rays;
  int R;
  float step, background, stop;
};

float t_of(const BakedRay& ray, float step, int k) { return fmaf((float)k + 0.5f, step, ray.near); }

// the point index of a cell's corner (0, 0, 0), restated: the dense grid, or the slot's 9 x 9 x 9 points
template <bool SPARSE>
int64_t corner_of(const Scene& S, const BakedSample& s, int64_t* sy, int64_t* sz) {
  if (!SPARSE) {
    *sy = S.G.sy, *sz = S.G.sz;
    return (int64_t)s.i[2] * S.G.sz + (int64_t)s.i[1] * S.G.sy + s.i[0];
  }
  const int64_t b = ((int64_t)(s.i[2] / 8) * S.dm.By + s.i[1] / 8) * S.dm.Bx + s.i[0] / 8;
  *sy = 9, *sz = 81;
  return (int64_t)S.slots[b] * 729 + ((s.i[2] % 8) * 9 + s.i[1] % 8) * 9 + s.i[0] % 8;
}

template <int DEG, bool SPARSE>
void run(const Scene& S, const void* points, int c0, const std::vector<int32_t>& K, const std::vector<size_t>& at,
         const std::vector<uint8_t>& flags, float* march, int32_t* brute, int32_t* count, std::vector<int32_t>& visit) {
  const BakedArgs A = {S.R, S.step, S.background, S.stop, points, SPARSE ? S.slots : nullptr, S.words, S.rays, nullptr, nullptr, nullptr};
  for (int bits = 0; bits < 2; ++bits) {
    const int c = c0 + bits;
    const uint8_t need = SPARSE ? (bits ? 13 : 9) : (bits ? 7 : 1);  // (a sparse march reads the slot, never the brick bit)
    for (int r = 0; r < S.R; ++r) {
      const float* row = S.rays + (size_t)r * 8;
      const BakedOut out = baked_march<DEG, SPARSE>(A, S.G, S.dm, row, bits != 0);
      float* m = march + ((size_t)c * S.R + r) * 5;
      m[0] = out.rgb[0], m[1] = out.rgb[1], m[2] = out.rgb[2], m[3] = out.depth, m[4] = out.opacity;

      const BakedRay ray(row, S.step);
      int32_t n_brute = 0, n_visit = 0;
      if (ray.ok) {
        const BakedCorner<DEG> pts(points, ray.d, ray.len);
        // brute force: every sample that counts, in order, until the transmittance ends the ray
        float T = 1.0f;
        const uint8_t* fl = flags.data() + at[r];
        for (int k = 0; k < K[r]; ++k) {
          if ((fl[k] & need) != need) continue;
          ++n_brute;
          if (S.stop > 0.0f) {
            const BakedSample s = baked_locate(S.G, ray.o, ray.d, ray.near, S.step, k);
            int64_t sy, sz;
            const int64_t base = corner_of<SPARSE>(S, s, &sy, &sz);
            T = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T).Tn;
            if (T < S.stop) break;
          }
        }
        // the walk: what it hands to visit
        T = 1.0f;
        int cursor = 0;
        auto record = [&](const BakedSample& s, int64_t base, int64_t sy, int64_t sz) {
          while (cursor < ray.K && t_of(ray, S.step, cursor) < s.t) ++cursor;
          visit.push_back(cursor < ray.K && t_of(ray, S.step, cursor) == s.t ? cursor : -1);  // (-1: a t that is no sample's)
          ++cursor;
          ++n_visit;
          if (S.stop > 0.0f) {
            T = baked_blend<DEG>(pts, s, base, sy, sz, ray.delta, T).Tn;
            return T < S.stop;
          }
          return false;
        };
        baked_walk<SPARSE>(S.words, SPARSE ? S.slots : nullptr, S.step, S.G, S.dm, ray, bits != 0, record);
      }
      brute[(size_t)c * S.R + r] = n_brute;
      count[(size_t)c * S.R + r] = n_visit;
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: baked_host DIR\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const Blob dims = read_exact(dir + "dims.bin", 5 * 4), params = read_exact(dir + "params.bin", 9 * 4);
  const int32_t* dv = (const int32_t*)dims.p;
  const float* pv = (const float*)params.p;
  Scene S;
  S.R = dv[3];
  const int n_bricks = dv[4];
  S.step = pv[6], S.background = pv[7], S.stop = pv[8];
  if (!occ_dims(dv[0], dv[1], dv[2], &S.dm) || S.R <= 0 || n_bricks < 0) {
    fprintf(stderr, "baked_host: bad dims\n");
    return 2;
  }
  const size_t n_points = (size_t)(dv[0] + 1) * (dv[1] + 1) * (dv[2] + 1);
  Blob points[3], pool[3];
  for (int deg = 0; deg < 3; ++deg) {
    points[deg] = read_exact(dir + "points" + std::to_string(deg) + ".bin", n_points * ((size_t)16 << deg));
    pool[deg] = read_exact(dir + "pool" + std::to_string(deg) + ".bin", (size_t)n_bricks * 729 * ((size_t)16 << deg));
  }
  const Blob slots = read_exact(dir + "slots.bin", (size_t)S.dm.bricks * 4);
  const Blob words = read_exact(dir + "words.bin", (size_t)(S.dm.fine_words + S.dm.brick_words) * 4);
  const Blob rays = read_exact(dir + "rays.bin", (size_t)S.R * 32);
  S.words = (const uint32_t*)words.p, S.slots = (const int32_t*)slots.p, S.rays = (const float*)rays.p;

  // the lattice as every entry point makes it
  upnerf_baked_render_args a = {};
  a.Cx = dv[0], a.Cy = dv[1], a.Cz = dv[2], a.R = S.R;
  for (int k = 0; k < 3; ++k) a.lo[k] = pv[k], a.hi[k] = pv[3 + k];
  a.step = S.step, a.background = S.background, a.stop = S.stop;
  a.rgbs = (const float*)points[0].p, a.words = S.words, a.rays = S.rays;
  OccDims dm2;
  if (!baked_lattice(&a, points[0].p, 16, &S.G, &dm2)) {
    fprintf(stderr, "baked_host: the lattice is refused\n");
    return 2;
  }

  // brute force over every sample: where it falls and what the bits and the table say of its cell
  std::vector<int32_t> K(S.R);
  std::vector<size_t> at(S.R);
  std::vector<uint8_t> flags;
  for (int r = 0; r < S.R; ++r) {
    const BakedRay ray(S.rays + (size_t)r * 8, S.step);
    K[r] = ray.K;
    at[r] = flags.size();
    for (int k = 0; k < ray.K; ++k) {
      const BakedSample s = baked_locate(S.G, ray.o, ray.d, ray.near, S.step, k);
      uint8_t f = 0;
      if (s.inside) {
        const int64_t b = ((int64_t)(s.i[2] / OCC_BRICK) * S.dm.By + s.i[1] / OCC_BRICK) * S.dm.Bx + s.i[0] / OCC_BRICK;
        const int64_t cell = ((int64_t)s.i[2] * S.dm.Cy + s.i[1]) * S.dm.Cx + s.i[0];
        f = 1 | (occ_bit(S.words + S.dm.fine_words, b) ? 2 : 0) | (occ_bit(S.words, cell) ? 4 : 0) | (S.slots[b] >= 0 ? 8 : 0);
      }
      flags.push_back(f);
    }
  }

  // one thread per (degree, layout): each writes its own rows of march, brute and count, and its own list of visits
  std::vector<float> march((size_t)12 * S.R * 5);
  std::vector<int32_t> brute((size_t)12 * S.R), count((size_t)12 * S.R), visits[6], visit;
  float* m = march.data();
  int32_t *b = brute.data(), *n = count.data();
  std::thread th[6] = {
      std::thread([&] { run<0, false>(S, points[0].p, 0, K, at, flags, m, b, n, visits[0]); }),
      std::thread([&] { run<0, true>(S, pool[0].p, 2, K, at, flags, m, b, n, visits[1]); }),
      std::thread([&] { run<1, false>(S, points[1].p, 4, K, at, flags, m, b, n, visits[2]); }),
      std::thread([&] { run<1, true>(S, pool[1].p, 6, K, at, flags, m, b, n, visits[3]); }),
      std::thread([&] { run<2, false>(S, points[2].p, 8, K, at, flags, m, b, n, visits[4]); }),
      std::thread([&] { run<2, true>(S, pool[2].p, 10, K, at, flags, m, b, n, visits[5]); }),
  };
  for (int i = 0; i < 6; ++i) th[i].join();
  for (int i = 0; i < 6; ++i) visit.insert(visit.end(), visits[i].begin(), visits[i].end());

  write_all(dir + "march.bin", march.data(), march.size() * 4);
  write_all(dir + "K.bin", K.data(), K.size() * 4);
  write_all(dir + "flags.bin", flags.data(), flags.size());
  write_all(dir + "brute.bin", brute.data(), brute.size() * 4);
  write_all(dir + "count.bin", count.data(), count.size() * 4);
  write_all(dir + "visit.bin", visit.data(), visit.size() * 4);
  for (int deg = 0; deg < 3; ++deg) free(points[deg].p), free(pool[deg].p);
  free(slots.p), free(words.p), free(rays.p), free(dims.p), free(params.p);
  return 0;
}
