// The host program of the visibility march (tests/test_baked_prune_cpu.py builds and runs it through tests/host/walk_host_build.py).
// It includes csrc/baked.hip unchanged and calls baked_visibility_ray, the __host__ __device__ function the kernel calls, with a
// recorder that is a plain max: no HIP call, no launch, no device.  Usage: baked_vis_host DIR.  The inputs are baked_host's
// (dims.bin, params.bin, points{0,1,2}.bin, pool{0,1,2}.bin, slots.bin, words.bin, rays.bin), each read into a heap buffer of
// exactly the file's size.  Written, with c = degree * 2 + use_bits:
//   vis_dense.bin  fp32 [6][(Cz+1)(Cy+1)(Cx+1)]     vis_pool.bin  fp32 [6][n_bricks][729]   (per copy: no face max)
// Every recorded index is checked against the array it goes to before it is used.
#include "baked.hip"

#include <stdio.h>
#include <stdlib.h>

#include <string>
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
    fprintf(stderr, "baked_vis_host: cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  b.n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  if (b.n != want) {
    fprintf(stderr, "baked_vis_host: %s has %zu bytes, not %zu\n", path.c_str(), b.n, want);
    exit(2);
  }
  if (posix_memalign(&b.p, 64, b.n ? b.n : 1) != 0 || (b.n && fread(b.p, 1, b.n, f) != b.n)) {
    fprintf(stderr, "baked_vis_host: cannot read %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
  return b;
}

void write_all(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, 1, n, f) != n) || fclose(f) != 0) {
    fprintf(stderr, "baked_vis_host: cannot write %s\n", path.c_str());
    exit(2);
  }
}

template <bool SPARSE>
void run(BakedVisArgs A, const BakedGrid& G, const OccDims& dm, bool use_bits, float* vis, size_t n) {
  auto record = [&](int64_t p, float m) {
    if (p < 0 || (size_t)p >= n || !(m > 0.0f) || !isfinite(m)) {
      fprintf(stderr, "baked_vis_host: recorded %g at %lld of %zu\n", (double)m, (long long)p, n);
      exit(3);
    }
    vis[p] = fmaxf(vis[p], m);
  };
  for (int r = 0; r < A.R; ++r) baked_visibility_ray<SPARSE>(A, G, dm, A.rays + (size_t)r * 8, use_bits, record);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: baked_vis_host DIR\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const Blob dims = read_exact(dir + "dims.bin", 5 * 4), params = read_exact(dir + "params.bin", 9 * 4);
  const int32_t* dv = (const int32_t*)dims.p;
  const float* pv = (const float*)params.p;
  OccDims dm;
  const int R = dv[3], n_bricks = dv[4];
  if (!occ_dims(dv[0], dv[1], dv[2], &dm) || R <= 0 || n_bricks < 0) {
    fprintf(stderr, "baked_vis_host: bad dims\n");
    return 2;
  }
  const size_t n_points = (size_t)(dv[0] + 1) * (dv[1] + 1) * (dv[2] + 1), n_pool = (size_t)n_bricks * 729;
  Blob points[3], pool[3];
  for (int deg = 0; deg < 3; ++deg) {
    points[deg] = read_exact(dir + "points" + std::to_string(deg) + ".bin", n_points * ((size_t)16 << deg));
    pool[deg] = read_exact(dir + "pool" + std::to_string(deg) + ".bin", n_pool * ((size_t)16 << deg));
  }
  const Blob slots = read_exact(dir + "slots.bin", (size_t)dm.bricks * 4);
  const Blob words = read_exact(dir + "words.bin", (size_t)(dm.fine_words + dm.brick_words) * 4);
  const Blob rays = read_exact(dir + "rays.bin", (size_t)R * 32);

  // the lattice as every entry point makes it
  upnerf_baked_render_args a = {};
  a.Cx = dv[0], a.Cy = dv[1], a.Cz = dv[2], a.R = R;
  for (int k = 0; k < 3; ++k) a.lo[k] = pv[k], a.hi[k] = pv[3 + k];
  a.step = pv[6], a.background = 0.0f, a.stop = pv[8];
  a.rgbs = (const float*)points[0].p, a.words = (const uint32_t*)words.p, a.rays = (const float*)rays.p;
  BakedGrid G;
  OccDims dm2;
  if (!baked_lattice(&a, points[0].p, 16, &G, &dm2)) {
    fprintf(stderr, "baked_vis_host: the lattice is refused\n");
    return 2;
  }

  std::vector<float> dense(6 * n_points, 0.0f), sparse(6 * n_pool, 0.0f);
  const int sigma_at[3] = {12, 24, 56};
  for (int deg = 0; deg < 3; ++deg)
    for (int bits = 0; bits < 2; ++bits) {
      const int c = deg * 2 + bits;
      BakedVisArgs A = {R, pv[6], pv[8], 16 << deg, sigma_at[deg], points[deg].p, nullptr, (const uint32_t*)words.p, (const float*)rays.p, nullptr};
      run<false>(A, G, dm, bits != 0, dense.data() + c * n_points, n_points);
      A.points = pool[deg].p, A.slots = (const int32_t*)slots.p;
      run<true>(A, G, dm, bits != 0, sparse.data() + c * n_pool, n_pool);
    }
  write_all(dir + "vis_dense.bin", dense.data(), dense.size() * 4);
  write_all(dir + "vis_pool.bin", sparse.data(), sparse.size() * 4);
  for (int deg = 0; deg < 3; ++deg) free(points[deg].p), free(pool[deg].p);
  free(slots.p), free(words.p), free(rays.p), free(dims.p), free(params.p);
  return 0;
}
