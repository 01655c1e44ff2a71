// Binding for the reference's voxeliser loop, used only by tests/golden/make_reference_golden.py, which passes the directory of the
// reference's point_cloud_ops.h as an include path (the reference's own .cc names eight arguments for nine parameters and does not
// compile).  The build goes to oracle/_ref/, which is not committed.
#include <pybind11/numpy.h>
#include "point_cloud_ops.h"

PYBIND11_MODULE(ref_voxel, m) {
  m.def("points_to_voxel", &points_to_voxel<float, 3>);
}
