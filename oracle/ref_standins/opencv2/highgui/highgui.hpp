// Stand-in for <opencv2/highgui/highgui.hpp>, written for this repository.  TEST INFRASTRUCTURE ONLY.
// The reference shows its difference image only when visualizeIterations is set, which the driver never sets: imshow and
// waitKey exist so that the reference's headers compile, and do nothing.
#ifndef PHOVO_REF_STANDIN_OPENCV_HIGHGUI
#define PHOVO_REF_STANDIN_OPENCV_HIGHGUI

#include "opencv2/imgproc/imgproc.hpp"

namespace cv
{
template< class T > inline void imshow( const std::string &, const Mat_< T > & ) {}
inline int waitKey( int = 0 ) { return -1; }
}

#endif
