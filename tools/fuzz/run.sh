#!/bin/bash
# AddressSanitizer + UBSan runs of the host code of the BAM side (no GPU): the one-shot inflater on valid, truncated and
# mutated deflate streams with exact-size buffers, the Huffman BGZF encoder against zlib's inflate, the CIGAR walk of
# rmr_ref_to_signal on random and hostile CIGARs, the batch forms of round 5 (rmr_ref_anchor_batch, rmr_orient_bases), the
# reference-anchor composition for either signal direction (rmr_ref_anchor_batch_dir against a scalar restatement), the
# set-order restatement of csrc/pyset_order.c and the MM / ML tokeniser of `validate from_modbams` on grammatical, truncated and
# mutated tag regions, and the FASTA packing arithmetic of `analyze pileup_modbams --ref` (the piece plan of rmr_ref_genome_load and
# the per-thread code of the pack kernel, csrc/rmr_ref_pack.h) on contigs at random line widths with planted violations, and the
# aux tag reader of `analyze pileup_modbams --partition-tag` (rmr_bam_aux_values) on aux regions of every field type, every
# truncation of them and random mutations, against a byte-by-byte restatement.
# From the repository root:
#   bash tools/fuzz/run.sh
set -e
cd "$(dirname "$0")"
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/rmr_inflate_asan inflate_asan.cpp -lz
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -I../../include -o /tmp/rmr_bgzf_asan bgzf_asan.cpp ../../remora_amd/csrc/bgzf_deflate.cpp -lz
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o /tmp/rmr_r2s_asan r2s_asan.cpp
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -o /tmp/rmr_batch_asan batch_asan.cpp
g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -o /tmp/rmr_reverse_anchor_asan reverse_anchor_asan.cpp
gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -o /tmp/rmr_setorder_asan setorder_asan.c ../../remora_amd/csrc/pyset_order.c
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -o /tmp/rmr_mod_tags_asan mod_tags_asan.cpp
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/rmr_ref_pack_asan ref_pack_asan.cpp
# (the sanitizer runtimes linked in: the program starts whatever libraries the environment loads in front of it)
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -o /tmp/rmr_aux_tag_asan aux_tag_asan.cpp
/tmp/rmr_inflate_asan
/tmp/rmr_bgzf_asan
/tmp/rmr_r2s_asan
/tmp/rmr_batch_asan
/tmp/rmr_reverse_anchor_asan
/tmp/rmr_setorder_asan
/tmp/rmr_mod_tags_asan
/tmp/rmr_ref_pack_asan
/tmp/rmr_aux_tag_asan
