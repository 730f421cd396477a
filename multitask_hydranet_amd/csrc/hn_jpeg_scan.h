// Records shared by the host scan preparation (hn_jpeg.hip: hn_jpeg_scan_prepare) and the device scan decode (hn_jpeg_scan.hip); mirrored by
// jpeg.py SCAN_DTYPE.  Semantics in DESIGN.md 4g.
#pragma once

#define JPEG_SCAN_SUBSEQ 128           // raw scan bytes per subsequence (= per thread of the scan kernels)
#define JPEG_SCAN_WINDOW 256           // subsequences per window of the synchronisation pass (= its workgroup size)

struct JpegScanHuff {                  // one Huffman table in the form the decoders read (1416 bytes)
    unsigned char look_n[512], look_v[512];     // 9-bit look-ahead: code length (0 = longer than 9 bits) and symbol
    int maxcode[17];                            // largest code of each length, -1 = none
    int valoff[17];                             // symbol index = code + valoff[length]
    unsigned char vals[256];
};
static_assert(sizeof(JpegScanHuff) == 1416, "JpegScanHuff layout is mirrored by jpeg.py");

struct JpegScanRec {                   // jpeg.py SCAN_DTYPE (8576 bytes)
    long scan_offset;                  // byte offset of the entropy-coded segment in the stream
    long scan_bytes;                   // its length up to and including EOI (or whatever marker ends it), or to the end of the data
    long stream_off;                   // byte offset of the stream in the batch's stream buffer (multiple of 16); pack_streams fills it
    long coef_off;                     // byte offset of the image's coefficients in coefs (multiple of 16);      pack_streams fills it
    int ncomp, hs, vs, mcus_x, mcus_y, restart_interval;        // JpegHead's
    int td[3], ta[3];                  // per component: index into dc[] / ac[]
    JpegScanHuff dc[3], ac[3];         // the distinct tables the scan selects, in order of first use
};
static_assert(sizeof(JpegScanRec) == 8576, "JpegScanRec layout is mirrored by jpeg.py");
