// The host program of the baked marcher's ray gradient (tests/test_baked_pose_cpu.py builds and runs it; tests/host/walk_host_build.py
// has the recipe).  It includes csrc/baked.hip unchanged and calls only its __host__ __device__ function baked_ray_grad and the host
// function that makes the lattice: no HIP call, no launch, no device.  Usage: baked_ray_host DIR.  Every file is raw little-endian,
// read into a heap buffer of exactly the file's size (an overread lands in a redzone of a sanitizer build).  Read: dims.bin,
// params.bin, points{0,1,2}.bin, pool{0,1,2}.bin, slots.bin, words.bin and rays.bin as baked_host.hip reads them, and
//   up.bin      fp32  [R][5]       the upstream gradients g_rgb | g_depth | g_opacity of each ray
// Written, with c = (degree * 2 + layout) * 2 + use_bits (layout 0 dense, 1 sparse):
//   grad.bin    fp32  [12][R][8]   baked_ray_grad: the gradient of o | d | near | far
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
    fprintf(stderr, "baked_ray_host: cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  b.n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  if (b.n != want) {
    fprintf(stderr, "baked_ray_host: %s has %zu bytes, not %zu\n", path.c_str(), b.n, want);
    exit(2);
  }
  if (posix_memalign(&b.p, 64, b.n ? b.n : 1) != 0 || (b.n && fread(b.p, 1, b.n, f) != b.n)) {
    fprintf(stderr, "baked_ray_host: cannot read %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
  return b;
}

template <int DEG, bool SPARSE>
void run(const BakedRayArgs& A, const BakedGrid& G, const OccDims& dm, const float* up, int c0, float* grad) {
  for (int bits = 0; bits < 2; ++bits)
    for (int r = 0; r < A.R; ++r) {
      const BakedRayGrad out = baked_ray_grad<DEG, SPARSE>(A, G, dm, A.rays + (size_t)r * 8, up + (size_t)r * 5, bits != 0);
      float* dst = grad + ((size_t)(c0 + bits) * A.R + r) * 8;
      for (int i = 0; i < 8; ++i) dst[i] = out.v[i];
    }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: baked_ray_host DIR\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const Blob dims = read_exact(dir + "dims.bin", 5 * 4), params = read_exact(dir + "params.bin", 9 * 4);
  const int32_t* dv = (const int32_t*)dims.p;
  const float* pv = (const float*)params.p;
  const int R = dv[3], n_bricks = dv[4];
  OccDims dm;
  if (!occ_dims(dv[0], dv[1], dv[2], &dm) || R <= 0 || n_bricks < 0) {
    fprintf(stderr, "baked_ray_host: bad dims\n");
    return 2;
  }
  const size_t n_points = (size_t)(dv[0] + 1) * (dv[1] + 1) * (dv[2] + 1);
  Blob points[3], pool[3];
  for (int deg = 0; deg < 3; ++deg) {
    points[deg] = read_exact(dir + "points" + std::to_string(deg) + ".bin", n_points * ((size_t)16 << deg));
    pool[deg] = read_exact(dir + "pool" + std::to_string(deg) + ".bin", (size_t)n_bricks * 729 * ((size_t)16 << deg));
  }
  const Blob slots = read_exact(dir + "slots.bin", (size_t)dm.bricks * 4);
  const Blob words = read_exact(dir + "words.bin", (size_t)(dm.fine_words + dm.brick_words) * 4);
  const Blob rays = read_exact(dir + "rays.bin", (size_t)R * 32), up = read_exact(dir + "up.bin", (size_t)R * 20);

  // the lattice as every entry point makes it
  upnerf_baked_render_args a = {};
  a.Cx = dv[0], a.Cy = dv[1], a.Cz = dv[2], a.R = R;
  for (int k = 0; k < 3; ++k) a.lo[k] = pv[k], a.hi[k] = pv[3 + k];
  a.step = pv[6], a.background = pv[7], a.stop = pv[8];
  a.rgbs = (const float*)points[0].p, a.words = (const uint32_t*)words.p, a.rays = (const float*)rays.p;
  BakedGrid G;
  OccDims dm2;
  if (!baked_lattice(&a, points[0].p, 16, &G, &dm2)) {
    fprintf(stderr, "baked_ray_host: the lattice is refused\n");
    return 2;
  }

  std::vector<float> grad((size_t)12 * R * 8);
  float* g = grad.data();
  const float* u = (const float*)up.p;
  auto args = [&](const void* pts, bool sparse) {
    return BakedRayArgs{R, a.step, a.background, a.stop, pts, sparse ? (const int32_t*)slots.p : nullptr, a.words, a.rays, nullptr, nullptr, nullptr, nullptr};
  };
  std::thread th[6] = {
      std::thread([&] { run<0, false>(args(points[0].p, false), G, dm, u, 0, g); }),
      std::thread([&] { run<0, true>(args(pool[0].p, true), G, dm, u, 2, g); }),
      std::thread([&] { run<1, false>(args(points[1].p, false), G, dm, u, 4, g); }),
      std::thread([&] { run<1, true>(args(pool[1].p, true), G, dm, u, 6, g); }),
      std::thread([&] { run<2, false>(args(points[2].p, false), G, dm, u, 8, g); }),
      std::thread([&] { run<2, true>(args(pool[2].p, true), G, dm, u, 10, g); }),
  };
  for (int i = 0; i < 6; ++i) th[i].join();

  FILE* f = fopen((dir + "grad.bin").c_str(), "wb");
  if (!f || fwrite(grad.data(), 4, grad.size(), f) != grad.size() || fclose(f) != 0) {
    fprintf(stderr, "baked_ray_host: cannot write grad.bin\n");
    return 2;
  }
  for (int deg = 0; deg < 3; ++deg) free(points[deg].p), free(pool[deg].p);
  free(slots.p), free(words.p), free(rays.p), free(up.p), free(dims.p), free(params.p);
  return 0;
}
