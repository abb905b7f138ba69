// Native sequence replay: drives mimosa_hip::replay::FixedLagReplay (host/mimosa_hip/replay.hpp) on an input file written
// by mimosa_amd/replay.py:write_native_input and prints one JSON object (estimated poses, per-stage seconds, scans/s).
//   replay_native <input.bin> [repeats] [manager | sequential | sharded <world> | sharded-rccl] [device-window[+photo-linear][+marginal | +marginal-joint] | device-window-relin=<rot>,<trans>[+photo-linear][+marginal | +marginal-joint]] [odometry] [device-poses]
//     device-poses (last word): replay::Config::device_poses — the per-timestamp deskew poses are computed on the device
//     device-window (in front of it): replay::Config::device_window — the smoother's iterations run as one chain of launches on
//       the device (FixedLagReplay without the photometric factor; refused elsewhere).  +photo-linear behind either form:
//       replay::Config::window_photo_linear — the photometric factor is accepted, linearized once per window call on the host
//       and carried by the chain as a linear factor.  +marginal behind all of that: replay::Config::window_marginal — the pose
//       that leaves the window is marginalised on the device and its marginal carried as the prior on the oldest pose;
//       +marginal-joint in its place: replay::Config::window_marginal_joint — with the odometry edges that reach from that pose
//       beyond pose 1, the marginal carried as the one joint factor of the window calls (needs odometry, every 1 .. 4 scans)
//     odometry (in front of device-poses, behind the window word): replay::Config::odometry_every — the input file ends with the
//       external odometry section (odometry_every; sigma_rot_deg, sigma_trans_m; per message scan index, pose, covariance); each
//       message goes through odometry::Manager and ties the window poses of two scans (FixedLagReplay; refused elsewhere)
//     repeats > 1: the whole sequence again, timing of the last pass is reported
//     sharded <world>: the map sharded over <world> ranks INSIDE this process (one host thread and one context each, in-process
//       transport: what a one-GPU box can run); sharded-rccl: this process is one rank of a torch.distributed.run-style launch
//       (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT), RCCL over xGMI.  The JSON carries rank 0's trajectory and
//       `max_rank_deviation_m`, the largest difference between any rank's positions and rank 0's (in-process form).
#include <cstdio>
#include <cstring>

#include "mimosa_hip/binio.hpp"
#include "mimosa_hip/replay.hpp"
#include "mimosa_hip/sharded_replay.hpp"

using namespace mimosa_hip;
using binio::read_vec;

int main(int argc, char ** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: replay_native <input.bin> [repeats] [manager | sequential | sharded <world> | sharded-rccl] [device-window[+photo-linear][+marginal | +marginal-joint] | device-window-relin=<rot>,<trans>[+photo-linear][+marginal | +marginal-joint]] [odometry] [device-poses]\n");
    return 2;
  }
  const bool device_poses = argc > 2 && std::string(argv[argc - 1]) == "device-poses";
  if (device_poses) --argc;
  // odometry: the input file ends with the external odometry section (replay::Config::odometry_every, the sigmas, the messages)
  const bool odometry = argc > 2 && std::string(argv[argc - 1]) == "odometry";
  if (odometry) --argc;
  // device-window-relin=<rot>,<trans>: device-window with replay::Config::window_relin (relinearization thresholds, rad and m)
  std::string window_word = argc > 2 ? argv[argc - 1] : "";
  const std::string joint_suffix = "+marginal-joint";
  const bool window_marginal_joint = window_word.size() > joint_suffix.size() && window_word.compare(window_word.size() - joint_suffix.size(), joint_suffix.size(), joint_suffix) == 0;
  if (window_marginal_joint) window_word.resize(window_word.size() - joint_suffix.size());
  const std::string marginal_suffix = "+marginal";
  const bool window_marginal = window_word.size() > marginal_suffix.size() && window_word.compare(window_word.size() - marginal_suffix.size(), marginal_suffix.size(), marginal_suffix) == 0;
  if (window_marginal) window_word.resize(window_word.size() - marginal_suffix.size());
  const std::string photo_suffix = "+photo-linear";
  const bool window_photo_linear = window_word.size() > photo_suffix.size() && window_word.compare(window_word.size() - photo_suffix.size(), photo_suffix.size(), photo_suffix) == 0;
  if (window_photo_linear) window_word.resize(window_word.size() - photo_suffix.size());
  bool device_window = window_word == "device-window";
  bool window_relin = false;
  double relin_rot = 0.0, relin_trans = 0.0;
  if (!device_window && std::sscanf(window_word.c_str(), "device-window-relin=%lf,%lf", &relin_rot, &relin_trans) == 2) device_window = window_relin = true;
  if (device_window) --argc;
  const int repeats = argc > 2 ? std::atoi(argv[2]) : 1;
  const bool through_manager = argc > 3 && std::string(argv[3]) == "manager";  // the same sequence through lidar::Manager::callback
  const bool sequential = argc > 3 && std::string(argv[3]) == "sequential";   // FixedLagReplay without the cross-scan overlap
  const bool sharded_local = argc > 4 && std::string(argv[3]) == "sharded";
  const bool sharded_rccl = argc > 3 && std::string(argv[3]) == "sharded-rccl";
  const int world = sharded_local ? std::atoi(argv[4]) : 1;
  try {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the input file");
    const auto I = read_vec<int32_t>(f);   // window, update_iters, photometric, neighbour mode, lru_horizon[, photo_window[, init_align iterations]]
    const auto D = read_vec<double>(f);    // between sigmas (rot, trans), keyframe thresholds (trans, rot deg), gravity xyz
    const auto regb = read_vec<uint8_t>(f);
    const auto inpb = read_vec<uint8_t>(f);
    if ((I.size() != 5 && I.size() != 6 && I.size() != 7) || D.size() != 7 || regb.size() != sizeof(mh_reg_config) || inpb.size() != sizeof(mh_input_config))
      throw std::runtime_error("configuration block has the wrong shape");
    replay::Config cfg;
    cfg.window = I[0];
    cfg.update_iters = I[1];
    cfg.photometric = I[2] != 0;
    cfg.photo_window = (I.size() > 5 ? I[5] : 0) != 0;
    cfg.init_align = I.size() > 6 && I[6] > 0;  // (the seventh word: init_align's iteration limit)
    if (cfg.init_align) cfg.init_align_iters = I[6];
    cfg.neighbor_voxel_mode = static_cast<size_t>(I[3]);
    cfg.between_sigma_rot = D[0];
    cfg.between_sigma_trans = D[1];
    cfg.keyframe_trans_thresh = D[2];
    cfg.keyframe_rot_thresh_deg = D[3];
    cfg.gravity = {D[4], D[5], D[6]};
    std::memcpy(&cfg.reg, regb.data(), sizeof(cfg.reg));
    std::memcpy(&cfg.input, inpb.data(), sizeof(cfg.input));
    if (cfg.photometric) cfg.photo = binio::read_photo_config(f);
    cfg.pipeline = !sequential;
    cfg.device_poses = device_poses;
    cfg.device_window = device_window;
    cfg.window_relin = window_relin;
    cfg.window_relin_rot = relin_rot;
    cfg.window_relin_trans = relin_trans;
    cfg.window_photo_linear = device_window && window_photo_linear;
    cfg.window_marginal = device_window && window_marginal;
    cfg.window_marginal_joint = device_window && window_marginal_joint;
    const auto bias = read_vec<double>(f);
    for (size_t i = 0; i + 2 < bias.size(); i += 3) cfg.bias_directions.push_back(V3D(bias[i], bias[i + 1], bias[i + 2]));
    const auto seed = read_vec<float>(f);
    const auto s0 = read_vec<double>(f);  // R (9), t (3), velocity (3): the state at the first IMU sample of the first sweep
    const auto nsc = read_vec<int32_t>(f);
    std::vector<replay::ScanInput> scans(static_cast<size_t>(nsc.at(0)));
    for (auto & sc : scans) {
      sc.raw = read_vec<lidar::PointOuster>(f);
      sc.imu.ts = read_vec<double>(f);
      const auto gy = read_vec<double>(f), ac = read_vec<double>(f);
      for (size_t j = 0; j < sc.imu.ts.size(); ++j) {
        sc.imu.gyro.push_back({gy[3 * j], gy[3 * j + 1], gy[3 * j + 2]});
        sc.imu.acc.push_back({ac[3 * j], ac[3 * j + 1], ac[3 * j + 2]});
      }
      sc.header_ts = read_vec<double>(f).at(0);
    }
    if (odometry) {
      const auto oe = read_vec<int32_t>(f);  // odometry_every
      const auto os = read_vec<double>(f);   // sigma_rot_deg, sigma_trans_m
      const auto om = read_vec<double>(f);   // per message: scan index, R (9), t (3), covariance (36, row-major)
      if (!f || oe.size() != 1 || oe[0] < 1 || os.size() != 2 || om.size() % 49) throw std::runtime_error("odometry: the input file has no odometry section");
      cfg.odometry_every = oe[0];
      cfg.odometry_sigma_rot_deg = os[0];
      cfg.odometry_sigma_trans_m = os[1];
      for (size_t j = 0; j < om.size() / 49; ++j) {
        const double * q = &om[49 * j];
        replay::ScanInput & sc = scans.at(static_cast<size_t>(q[0]));
        sc.has_odometry = true;
        for (int i = 0; i < 9; ++i) sc.odometry_T.R[i] = q[1 + i];
        for (int i = 0; i < 3; ++i) sc.odometry_T.t[i] = q[10 + i];
        for (int i = 0; i < 36; ++i) sc.odometry_cov[i] = q[13 + i];
      }
    }
    replay::State st0;
    if (s0.size() < 15) throw std::runtime_error("the initial state needs 15 doubles");
    for (int i = 0; i < 9; ++i) st0.T.R[i] = s0[i];
    for (int i = 0; i < 3; ++i) st0.T.t[i] = s0[9 + i];
    st0.vel = {s0[12], s0[13], s0[14]};
    const char * lr = std::getenv("LOCAL_RANK");
    auto ctx = std::make_shared<lidar::Context>(sharded_rccl && lr ? std::atoi(lr) : 0);
    replay::Result r;
    double max_dev = 0.0;
    int n_ranks = 1;
    for (int rep = 0; rep < repeats; ++rep) {
      if (sharded_local) {
        // `world` ranks = host threads of this process, one context each on the one device
        if (world < 1 || world > 64) throw std::runtime_error("sharded: world in 1..64");
        n_ranks = world;
        std::vector<std::shared_ptr<lidar::Context>> ctxs{ctx};
        for (int q = 1; q < world; ++q) ctxs.push_back(std::make_shared<lidar::Context>(0));
        const auto comms = lidar::ShardCommunicator::local(ctxs);
        std::vector<replay::Result> rr(static_cast<size_t>(world));
        std::vector<std::string> err(static_cast<size_t>(world));
        std::vector<std::thread> th;
        for (int q = 0; q < world; ++q)
          th.emplace_back([&, q] {
            try {
              replay::ShardedFixedLagReplay run(comms[static_cast<size_t>(q)], cfg, static_cast<size_t>(I[4]), 3, world == 1);
              run.seedMap(seed.data(), seed.size() / 3);
              rr[static_cast<size_t>(q)] = run.run(scans, st0);
            } catch (const std::exception & e) {
              err[static_cast<size_t>(q)] = e.what();
            }
          });
        for (auto & t : th) t.join();
        for (int q = 0; q < world; ++q)
          if (!err[static_cast<size_t>(q)].empty()) throw std::runtime_error("rank " + std::to_string(q) + ": " + err[static_cast<size_t>(q)]);
        r = rr[0];
        max_dev = 0.0;
        for (int q = 1; q < world; ++q) {
          r.seconds = std::max(r.seconds, rr[static_cast<size_t>(q)].seconds);
          for (size_t k = 0; k < r.poses.size(); ++k)
            for (int i = 0; i < 3; ++i) max_dev = std::max(max_dev, std::fabs(rr[static_cast<size_t>(q)].poses[k].t[i] - r.poses[k].t[i]));
        }
      } else if (sharded_rccl) {
        const auto comm = lidar::ShardCommunicator::rcclFromEnv(ctx);
        n_ranks = comm->world();
        replay::ShardedFixedLagReplay run(comm, cfg, static_cast<size_t>(I[4]), 3, comm->world() == 1);
        run.seedMap(seed.data(), seed.size() / 3);
        r = run.run(scans, st0);
      } else if (through_manager) {
        replay::ManagerReplay run(ctx, cfg, static_cast<size_t>(I[4]));
        r = run.run(scans, st0, seed.data(), seed.size() / 3);
      } else {
        replay::FixedLagReplay run(ctx, cfg, static_cast<size_t>(I[4]));
        run.seedMap(seed.data(), seed.size() / 3);
        r = run.run(scans, st0);
      }
    }
    std::printf("{\"scans\": %zu, \"seconds\": %.9f, \"scans_per_s\": %.3f, \"n_keyframes\": %d, \"n_ranks\": %d, \"max_rank_deviation_m\": %.3e, \"device_pose_scans\": %d,\n", scans.size(),
                r.seconds, static_cast<double>(scans.size()) / r.seconds, r.n_keyframes, n_ranks, max_dev, r.device_pose_scans);
    std::printf("\"stage_s\": {\"front_end\": %.9f, \"imu\": %.9f, \"factor_create\": %.9f, \"optimise\": %.9f, \"update_map\": %.9f},\n",
                r.stage[0], r.stage[1], r.stage[2], r.stage[3], r.stage[4]);
    {
      const char * names[12] = {"stage_wait", "prepare_incl_stage_wait", "deskew", "geo_preprocess", "icp_create", "photo_wait", "photo_preprocess", "photo_factor",
                                "optimise", "keyframe_map", "photo_final_linearize", "photo_tail_incl_final_linearize"};
      std::printf("\"detail_s\": {");
      for (int i = 0; i < 12; ++i) std::printf("\"%s\": %.9f, ", names[i], r.detail[i]);
      std::printf("\"stager_start_latency\": %.9f, \"stager_prefetch\": %.9f, \"photo_worker_start_latency\": %.9f, \"photo_worker_update_map\": %.9f},\n", r.worker[0],
                  r.worker[1], r.worker[2], r.worker[3]);
    }
    std::printf("\"photo_valid\": [");
    for (size_t i = 0; i < r.photo_valid.size(); ++i) std::printf("%d%s", r.photo_valid[i], i + 1 < r.photo_valid.size() ? ", " : "");
    std::printf("],\n\"photo_in_window\": [");
    for (size_t i = 0; i < r.photo_in_window.size(); ++i) std::printf("%d%s", r.photo_in_window[i], i + 1 < r.photo_in_window.size() ? ", " : "");
    std::printf("],\n\"marginal_valid\": [");
    for (size_t i = 0; i < r.marginal_valid.size(); ++i) std::printf("%d%s", r.marginal_valid[i], i + 1 < r.marginal_valid.size() ? ", " : "");
    std::printf("],\n\"separator_sizes\": [");
    for (size_t i = 0; i < r.separator_sizes.size(); ++i) std::printf("%d%s", r.separator_sizes[i], i + 1 < r.separator_sizes.size() ? ", " : "");
    std::printf("],\n\"init_align_iters\": %d,\n\"first_costs\": [", r.init_align_iters);
    for (size_t i = 0; !r.costs.empty() && i < r.costs.at(0).size(); ++i) std::printf("%.17g%s", r.costs[0][i], i + 1 < r.costs[0].size() ? ", " : "");
    std::printf("],\n\"poses\": [");
    for (size_t k = 0; k < r.poses.size(); ++k) {
      std::printf("[");
      for (int i = 0; i < 9; ++i) std::printf("%.17g, ", r.poses[k].R[i]);
      std::printf("%.17g, %.17g, %.17g]%s", r.poses[k].t[0], r.poses[k].t[1], r.poses[k].t[2], k + 1 < r.poses.size() ? ", " : "");
    }
    std::printf("]}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "replay_native: %s\n", e.what());
    return 1;
  }
  return 0;
}
