// gtsam_sig: stand-in for <gtsam/navigation/ImuBias.h>: imuBias::ConstantBias with the accessors DopplerHessianFactor reads
// (include/mimosa/radar/factor.hpp:105-111).  NOT GTSAM.
#pragma once
#include <gtsam/base/Vector.h>

namespace gtsam
{
namespace imuBias
{
class ConstantBias
{
public:
  ConstantBias() : acc_(Vector3::Zero()), gyro_(Vector3::Zero()) {}
  ConstantBias(const Vector3 & biasAcc, const Vector3 & biasGyro) : acc_(biasAcc), gyro_(biasGyro) {}
  const Vector3 & accelerometer() const { return acc_; }
  const Vector3 & gyroscope() const { return gyro_; }

private:
  Vector3 acc_, gyro_;
};
}  // namespace imuBias
}  // namespace gtsam
