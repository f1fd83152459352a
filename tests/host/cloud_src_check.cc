// csrc/cloud_src.h on the host: what CloudSrc carries, the copy kind it names, and the rule that a call's clouds lie in one place.
#include <cstdio>
#include <vector>

#include "cloud_src.h"

using lio::CloudSrc;

static int failed = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failed; } } while (0)

template <class F> static bool throws_logic_error(F f) {
  try { f(); } catch (const std::logic_error &) { return true; }
  return false;
}

int main() {
  static_assert(sizeof(float4) == 4 * sizeof(float), "a point is four floats");
  float pts[3 * 4] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  const float4 *as4 = reinterpret_cast<const float4 *>(pts);

  // host() and device() carry pointer, count and place
  const CloudSrc h = CloudSrc::host(pts, 3);
  CHECK(h.p == as4 && h.n == 3 && !h.on_device);
  CHECK(h.p[2].x == 8.f && h.p[2].w == 11.f);
  const CloudSrc d = CloudSrc::device(as4 + 1, 2);
  CHECK(d.p == as4 + 1 && d.n == 2 && d.on_device);
  const CloudSrc a0 = CloudSrc::at(pts, 3, false), a1 = CloudSrc::at(pts, 3, true);
  CHECK(a0.p == as4 && a0.n == 3 && !a0.on_device);
  CHECK(a1.p == as4 && a1.n == 3 && a1.on_device);

  // the empty cloud
  const CloudSrc e = CloudSrc::host(nullptr, 0);
  CHECK(e.p == nullptr && e.n == 0 && !e.on_device);
  const CloudSrc none = CloudSrc();
  CHECK(none.p == nullptr && none.n == 0 && !none.on_device);

  // the two copy kinds
  CHECK(h.to_device() == hipMemcpyHostToDevice && e.to_device() == hipMemcpyHostToDevice);
  CHECK(d.to_device() == hipMemcpyDeviceToDevice);

  // one place per call
  const std::vector<CloudSrc> all_host = {h, e, h}, all_dev = {d, CloudSrc::device(nullptr, 0), d};
  CHECK(!lio::clouds_on_device(all_host.data(), all_host.size()));
  CHECK(lio::clouds_on_device(all_dev.data(), all_dev.size()));
  CHECK(!lio::clouds_on_device(nullptr, 0));
  CHECK(!lio::clouds_on_device(&h, 1) && lio::clouds_on_device(&d, 1));
  const std::vector<CloudSrc> mix_a = {h, d}, mix_b = {d, d, e}, mix_c = {h, h, h, d};
  for (const std::vector<CloudSrc> *m : {&mix_a, &mix_b, &mix_c})
    CHECK(throws_logic_error([&] { lio::clouds_on_device(m->data(), m->size()); }));
  // ... and over clouds that do not lie in one array (the chains' records)
  struct Pair { CloudSrc corner; int between; CloudSrc surf; };
  const Pair same[2] = {{d, 0, d}, {d, 0, d}}, mixed[2] = {{d, 0, d}, {d, 0, h}};
  const auto of = [](const Pair *p) { return [p](size_t i) { return i & 1 ? p[i / 2].surf : p[i / 2].corner; }; };
  CHECK(lio::clouds_on_device(4, of(same)));
  CHECK(throws_logic_error([&] { lio::clouds_on_device(4, of(mixed)); }));
  CHECK(!lio::clouds_on_device(0, of(mixed)));

  if (failed) return 1;
  std::printf("cloud_src: OK\n");
  return 0;
}
