// Stand-in for <opencv2/contrib/contrib.hpp>, written for this repository.  TEST INFRASTRUCTURE ONLY.
// The reference uses cv::TickMeter only inside its console-progress blocks, which are compiled out; the class exists so
// that the include resolves.
#ifndef PHOVO_REF_STANDIN_OPENCV_CONTRIB
#define PHOVO_REF_STANDIN_OPENCV_CONTRIB

namespace cv
{
class TickMeter
{
public:
  void start() {}
  void stop() {}
  double getTimeSec() const { return 0.0; }
};
}

#endif
