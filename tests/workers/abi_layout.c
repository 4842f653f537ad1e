/* Prints what the C compiler makes of the three structs of include/t2i_hip.h: "<struct> sizeof <bytes>" and "<struct> <field> <offset>"
 * lines, in declared order.  tests/test_abi.py builds it with the host clang and holds the ctypes classes of _lib.py against it. */
#include <stddef.h>
#include <stdio.h>

#include "t2i_hip.h"

#define SIZE(T) printf(#T " sizeof %zu\n", sizeof(T))
#define FIELD(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))

int main(void) {
  SIZE(t2i_conv_desc);
  FIELD(t2i_conv_desc, B); FIELD(t2i_conv_desc, H); FIELD(t2i_conv_desc, W); FIELD(t2i_conv_desc, Cin);
  FIELD(t2i_conv_desc, Ho); FIELD(t2i_conv_desc, Wo); FIELD(t2i_conv_desc, Cout);
  FIELD(t2i_conv_desc, KH); FIELD(t2i_conv_desc, KW); FIELD(t2i_conv_desc, SH); FIELD(t2i_conv_desc, SW);
  FIELD(t2i_conv_desc, pad_t); FIELD(t2i_conv_desc, pad_l); FIELD(t2i_conv_desc, math);
  SIZE(t2i_conv_opts);
  FIELD(t2i_conv_opts, a_image); FIELD(t2i_conv_opts, b_image); FIELD(t2i_conv_opts, out_image); FIELD(t2i_conv_opts, xform);
  FIELD(t2i_conv_opts, xform_bytes); FIELD(t2i_conv_opts, xform_mode); FIELD(t2i_conv_opts, out_image_written);
  FIELD(t2i_conv_opts, xform_kept); FIELD(t2i_conv_opts, in_dtype); FIELD(t2i_conv_opts, out_dtype);
  FIELD(t2i_conv_opts, xform_valid_rows); FIELD(t2i_conv_opts, xform_plane_rows); FIELD(t2i_conv_opts, reserved);
  SIZE(t2i_image_desc);
  FIELD(t2i_image_desc, offset); FIELD(t2i_image_desc, height); FIELD(t2i_image_desc, width); FIELD(t2i_image_desc, channels);
  FIELD(t2i_image_desc, y1); FIELD(t2i_image_desc, y2); FIELD(t2i_image_desc, x1); FIELD(t2i_image_desc, x2);
  FIELD(t2i_image_desc, reserved);
  return 0;
}
