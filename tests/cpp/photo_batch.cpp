// Drives PhotometricFactor::linearizeBatch / linearizeBatchAsync of the C++ host mirror
// (mimosa_amd/host/mimosa_hip/photometric.hpp) on a window of photometric factors, one per frame, built through the
// reference's call order (preprocess -> getFactors -> linearize -> updateMap), and compares them with a loop of
// linearize() at the same Values, bit for bit.  Inputs are written by tests/test_gpu_photo_batch.py (the format of
// tests/cpp/photo_pipeline.cpp); argv[2] = number of frames.  Prints JSON.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "../../mimosa_amd/host/mimosa_hip/binio.hpp"

using namespace mimosa_hip;
using namespace mimosa_hip::lidar;
using mimosa_hip::binio::read_vec;

static bool same_bits(const double a, const double b) { return !std::memcmp(&a, &b, sizeof(double)); }

static bool same_hessian(const HessianFactor & a, const HessianFactor & b)
{
  const gtsam::Matrix Ga = a.information(), Gb = b.information();
  const gtsam::Vector ga = a.linearTerm(), gb = b.linearTerm();
  if (Ga.rows() != Gb.rows() || Ga.cols() != Gb.cols() || ga.size() != gb.size()) return false;
  for (int r = 0; r < Ga.rows(); ++r)
    for (int c = 0; c < Ga.cols(); ++c)
      if (!same_bits(Ga(r, c), Gb(r, c))) return false;
  for (int r = 0; r < ga.size(); ++r)
    if (!same_bits(ga(r), gb(r))) return false;
  return same_bits(a.constantTerm(), b.constantTerm());
}

// every field of mh_photo_result but the timing
static bool same_result(const mh_photo_result & a, const mh_photo_result & b)
{
#define MH_SAME(x) (!std::memcmp(&a.x, &b.x, sizeof(a.x)))
  return MH_SAME(H_bb) && MH_SAME(H_ba) && MH_SAME(H_aa) && MH_SAME(b_b) && MH_SAME(b_a) && MH_SAME(f) && MH_SAME(loc_trans_final) &&
         MH_SAME(loc_rot_final) && MH_SAME(eigvec_trans) && MH_SAME(eigvec_rot) && MH_SAME(status_hist) && MH_SAME(n_exceptions);
#undef MH_SAME
}

int main(int argc, char ** argv)
{
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const int n_frames = std::atoi(argv[2]);
  const PhotometricConfig cfg = binio::read_photo_config(f);
  const auto bias = read_vec<double>(f);
  std::vector<V3D> bias_directions;
  for (size_t i = 0; i + 2 < bias.size(); i += 3) bias_directions.push_back(V3D(bias[i], bias[i + 1], bias[i + 2]));
  try {
    auto ctx = std::make_shared<Context>(0);
    Photometric photo(ctx, cfg);
    Values values;
    std::vector<PhotometricFactor::Ptr> window;
    for (int k = 0; k < n_frames; ++k) {
      auto raw = read_vec<Point>(f);
      auto desk = read_vec<Point>(f);
      const auto ns = read_vec<uint32_t>(f);
      const auto T = read_vec<double>(f);
      const auto pose = read_vec<double>(f);
      std::vector<std::pair<uint32_t, Pose3>> interp(ns.size());
      for (size_t g = 0; g < ns.size(); ++g) interp[g] = {ns[g], pose3(&T[12 * g], &T[12 * g + 9])};
      const Key Xk = X(10 + k);
      values.insert(Xk, pose3(pose.data(), pose.data() + 9));
      photo.preprocess(raw, desk, interp, 0.1 * k, Xk);
      NonlinearFactorGraph graph;
      photo.getFactors(values, graph);
      if (!graph.empty()) {
        graph.at(0)->linearize(values);  // updateMap reads this linearize's statuses
        window.push_back(photo.factor());
      }
      photo.updateMap(values, bias_directions);
    }
    // the smoother's next iterate: every pose moved a little
    Values moved;
    for (int k = 0; k < n_frames; ++k) {
      const Pose3 p = values.at<Pose3>(X(10 + k));
      const PoseRM q = rowMajor(p);
      double t[3] = {q.t[0] + 0.01 * (k + 1), q.t[1] - 0.005 * k, q.t[2] + 0.002};
      moved.insert(X(10 + k), pose3(q.R.data(), t));
    }
    int equal = 1, async_equal = 1, valid = 0;
    for (const Values * v : {&values, &moved}) {
      std::vector<std::shared_ptr<GaussianFactor>> single;
      std::vector<mh_photo_result> single_r;
      std::vector<std::vector<PhotometricFactor::RejectStatus>> single_s;
      std::vector<std::vector<std::array<double, 2>>> single_c;
      for (const auto & x : window) {
        single.push_back(x->linearize(*v));
        single_r.push_back(x->lastResult());
        single_s.push_back(x->getStatuses());
        single_c.push_back(x->getCenters());
        valid += single_r.back().status_hist[8];
      }
      const auto batch = PhotometricFactor::linearizeBatch(window, *v);
      for (size_t i = 0; i < window.size(); ++i) {
        equal &= same_hessian(*std::static_pointer_cast<HessianFactor>(batch[i]), *std::static_pointer_cast<HessianFactor>(single[i]));
        equal &= same_result(window[i]->lastResult(), single_r[i]);
        equal &= window[i]->getStatuses() == single_s[i];
        const auto c = window[i]->getCenters();
        equal &= c.size() == single_c[i].size() && (c.empty() || !std::memcmp(c.data(), single_c[i].data(), c.size() * sizeof(c[0])));
      }
      PhotometricFactor::linearizeBatchAsync(window, *v);
      for (size_t i = window.size(); i-- > 0;) {  // collected in reverse order
        const auto h = window[i]->collect();
        async_equal &= same_hessian(*std::static_pointer_cast<HessianFactor>(h), *std::static_pointer_cast<HessianFactor>(single[i]));
        async_equal &= same_result(window[i]->lastResult(), single_r[i]);
      }
    }
    std::printf("{\"n_factors\": %zu, \"n_valid\": %d, \"equal\": %d, \"async_equal\": %d}\n", window.size(), valid, equal, async_equal);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "photo_batch: %s\n", e.what());
    return 1;
  }
  return 0;
}
