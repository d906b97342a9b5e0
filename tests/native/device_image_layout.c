/* Prints the layout of phovo_device_image and phovo_ingest_record as a C11 compiler sees include/phovo_hip.h, and checks
 * that the device-ingest entry points refuse a NULL engine loudly (no GPU needed).  tests/test_device_ingest_cpu.py compares
 * the printed numbers with the ctypes declarations of native.py.  Exit code 0 = the refusals behaved. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "phovo_hip.h"

int main(void)
{
  printf("device_image size %zu data %zu row_stride_bytes %zu frame_stride_bytes %zu format %zu reserved %zu\n",
         sizeof(phovo_device_image), offsetof(phovo_device_image, data), offsetof(phovo_device_image, row_stride_bytes),
         offsetof(phovo_device_image, frame_stride_bytes), offsetof(phovo_device_image, format),
         offsetof(phovo_device_image, reserved));
  printf("ingest_record size %zu chunks %zu wide_launches %zu scalar_launches %zu reserved %zu\n",
         sizeof(phovo_ingest_record), offsetof(phovo_ingest_record, chunks), offsetof(phovo_ingest_record, wide_launches),
         offsetof(phovo_ingest_record, scalar_launches), offsetof(phovo_ingest_record, reserved));
  printf("formats %d %d %d %d %d %d %d\n", PHOVO_IMAGE_U8_GRAY, PHOVO_IMAGE_U8_RGB, PHOVO_IMAGE_U8_BGR, PHOVO_IMAGE_F64,
         PHOVO_IMAGE_F32, PHOVO_IMAGE_F16, PHOVO_IMAGE_U16);
  phovo_device_image img;
  memset(&img, 0, sizeof(img));
  phovo_ingest_record rec;
  int bad = 0;
  bad += phovo_engine_upload_frames_device(NULL, 0, 1, PHOVO_ROLE_BOTH, &img, &img, 1.0, NULL) != PHOVO_E_INVALID_ARGUMENT;
  bad += strstr(phovo_last_error(), "null engine") == NULL;
  bad += phovo_engine_last_ingest(NULL, &rec) != PHOVO_E_INVALID_ARGUMENT;
  bad += phovo_odometry_set_source_frame_device(NULL, &img, &img, 1.0, 4, 4, NULL) != PHOVO_E_INVALID_ARGUMENT;
  bad += phovo_odometry_set_target_frame_device(NULL, &img, NULL, 1.0, 4, 4, NULL) != PHOVO_E_INVALID_ARGUMENT;
  bad += strstr(phovo_last_error(), "null odometry") == NULL;
  printf("null refusals %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
