/* Prototypes of the entry points added since the memory-contract case table of the test suite was last brought up to
 * date.  Included by ru3d.h, inside its extern "C" block and behind the section that states each contract; never
 * included on its own.  _native.SIGNATURES_SINCE binds exactly the functions declared here, as _native.SIGNATURES binds
 * those of ru3d.h.  A later tests-only change moves both back into ru3d.h and SIGNATURES together with cases in the
 * table, and this file goes away. */
#ifndef RU3D_H
#error "include ru3d.h, which includes this file"
#endif

/* local thickness (the section of that name in ru3d.h) */
size_t ru3d_thickness_workspace_bytes(int X, int Y, int Z);
int ru3d_thickness_candidates(const uint64_t* bits, int X, int Y, int Z, int32_t* index, int64_t capacity, int64_t* count,
                              void* ws, size_t ws_bytes, void* stream);
int ru3d_thickness_paint(const double* r2, const int32_t* index, int64_t n, int X, int Y, int Z, const double* spacing,
                         double* out, int64_t* work_dev, void* stream);
