# Builds the gfx950 C-ABI library (flope_amd/lib/libflope_amd.so) and the CPU-only
# host test harness (tests/host_harness/libflope_host_harness.so).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := flope_amd/csrc
OBJDIR   := build/obj
LIB      := flope_amd/lib/libflope_amd.so
HARNESS  := tests/host_harness/libflope_host_harness.so
HARNESS_F32M := tests/host_harness/libflope_host_f32m.so
HARNESS_F32M_KSPLIT := tests/host_harness/libflope_host_f32m_ksplit.so
HARNESS_GUARD := tests/host_harness/libflope_host_guard.so
HARNESS_TF_F32M := tests/host_harness/libflope_host_tf_f32m.so
HARNESS_TF_ATTN := tests/host_harness/libflope_host_tf_attn.so
HARNESS_TF_VARLEN := tests/host_harness/libflope_host_tf_varlen.so
HARNESS_TF_FUSED := tests/host_harness/libflope_host_tf_fused.so
HARNESS_TF_CAUSAL := tests/host_harness/libflope_host_tf_causal.so
HARNESS_TF_STREAM := tests/host_harness/libflope_host_tf_stream.so
HARNESS_TF_WINDOW := tests/host_harness/libflope_host_tf_window.so
HARNESS_TF_WINDOW16 := tests/host_harness/libflope_host_tf_window16.so
HARNESS_TF_EXTEND := tests/host_harness/libflope_host_tf_extend.so
HARNESS_TF_SPLIT := tests/host_harness/libflope_host_tf_split.so
HARNESS_TF_EXTEND16 := tests/host_harness/libflope_host_tf_extend16.so
HARNESS_TF_MASK := tests/host_harness/libflope_host_tf_mask.so
HARNESS_TF_MASK16 := tests/host_harness/libflope_host_tf_mask16.so
HARNESS_TF_BIAS := tests/host_harness/libflope_host_tf_bias.so
HARNESS_TF_STREAM_BIAS := tests/host_harness/libflope_host_tf_stream_bias.so
HARNESS_TF_BIAS16 := tests/host_harness/libflope_host_tf_bias16.so
HARNESS_DEPTH := tests/host_harness/libflope_host_depth.so
HARNESS_CROP := tests/host_harness/libflope_host_crop.so
HARNESS_FRAME := tests/host_harness/libflope_host_frame.so
HARNESS_TRACK := tests/host_harness/libflope_host_track.so
HARNESS_TF_FEED := tests/host_harness/libflope_host_tf_feed.so
HARNESS_TF_SKINNY := tests/host_harness/libflope_host_tf_skinny.so
HARNESS_TF_SKINNY_LN := tests/host_harness/libflope_host_tf_skinny_ln.so
HARNESS_TF_ARCH := tests/host_harness/libflope_host_tf_arch.so
SRCS    := $(wildcard $(CSRC)/*.hip)
OBJS     := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS))
HDRS     := $(wildcard $(CSRC)/*.h) include/flope_amd.h
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wno-unused-value -Iinclude

all: $(LIB) $(HARNESS) $(HARNESS_F32M) $(HARNESS_F32M_KSPLIT) $(HARNESS_GUARD) $(HARNESS_TF_F32M) $(HARNESS_TF_ATTN) $(HARNESS_TF_VARLEN) $(HARNESS_TF_FUSED) $(HARNESS_TF_CAUSAL) $(HARNESS_TF_STREAM) $(HARNESS_TF_WINDOW) $(HARNESS_TF_WINDOW16) $(HARNESS_TF_EXTEND) $(HARNESS_TF_SPLIT) $(HARNESS_TF_EXTEND16) $(HARNESS_TF_MASK) $(HARNESS_TF_MASK16) $(HARNESS_TF_BIAS) $(HARNESS_TF_STREAM_BIAS) $(HARNESS_TF_BIAS16) $(HARNESS_DEPTH) $(HARNESS_CROP) $(HARNESS_FRAME) $(HARNESS_TRACK) $(HARNESS_TF_FEED) $(HARNESS_TF_SKINNY) $(HARNESS_TF_SKINNY_LN) $(HARNESS_TF_ARCH)

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

$(HARNESS): tests/host_harness/harness.cpp $(CSRC)/pose_math.h $(CSRC)/host_pack.h $(CSRC)/w4_sched.h $(CSRC)/plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# packers and operand feed of the float32 MFMA trunk (tests/test_f32m_host.py)
$(HARNESS_F32M): tests/host_harness/harness_f32m.cpp $(CSRC)/host_pack.h $(CSRC)/w4_sched.h $(CSRC)/plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# planner helpers and the split launch + finalize walk of the float32 MFMA trunk's split-K form (tests/test_f32m_ksplit_host.py,
# tests/test_gpu_f32m_ksplit.py); linked with harness_f32m.cpp, whose walk is the S = 1 case
$(HARNESS_F32M_KSPLIT): tests/host_harness/harness_f32m_ksplit.cpp tests/host_harness/harness_f32m.cpp $(CSRC)/host_pack.h $(CSRC)/w4_sched.h $(CSRC)/plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ tests/host_harness/harness_f32m_ksplit.cpp tests/host_harness/harness_f32m.cpp

# packer and operand feed of the float32 MFMA encoder linear (tests/test_tf_f32m_host.py, tests/test_gpu_tf_f32m.py)
$(HARNESS_TF_F32M): tests/host_harness/harness_tf_f32m.cpp $(CSRC)/host_pack.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# attention kernel selection of the encoder and the constants of its launches (tests/test_tf_attn_plan_host.py,
# tests/test_gpu_tf_attn_tiled.py)
$(HARNESS_TF_ATTN): tests/host_harness/harness_tf_attn.cpp $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# ragged-batch planner of the encoder: offsets, limits and the variable-length attention launches (tests/test_tf_varlen_host.py,
# tests/test_gpu_tf_varlen.py)
$(HARNESS_TF_VARLEN): tests/host_harness/harness_tf_varlen.cpp $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# planner of the encoder's single-launch forward (LDS layout, summation-order rule, eligibility) and a scalar walk of the kernel
# through that layout with every index checked (tests/test_tf_fused_host.py, tests/test_gpu_tf_fused.py)
$(HARNESS_TF_FUSED): tests/host_harness/harness_tf_fused.cpp $(CSRC)/tf_fused_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# how far causal attention walks the keys: the planner's constexpr functions the four attention kernels call
# (tests/test_tf_causal_host.py, tests/test_gpu_tf_causal.py)
$(HARNESS_TF_CAUSAL): tests/host_harness/harness_tf_causal.cpp $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the streaming forward's planner: argument checks of step / prefill / reset, the capacity limit, the launches of tf_attn_step and
# tf_cache_append (tests/test_tf_stream_host.py, tests/test_gpu_tf_stream.py)
$(HARNESS_TF_STREAM): tests/host_harness/harness_tf_stream.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# sliding-window causal attention and the ring cache of a windowed stream state: the first visible key, the slot of a position, the
# row runs of a step, the rows a fill writes, the windowed checks (tests/test_tf_window_host.py, tests/test_gpu_tf_window.py)
$(HARNESS_TF_WINDOW): tests/host_harness/harness_tf_window.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the window on the 16-bit MFMA attention kernels: the first step of a wave, the steps it takes, the first block a workgroup loads,
# the pick under a window (tests/test_tf_window16_host.py, tests/test_gpu_tf_window16.py)
$(HARNESS_TF_WINDOW16): tests/host_harness/harness_tf_window16.cpp $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the planner of flope_tf_stream_extend: its checks on linear and windowed states, the per-sequence table, the launches of
# tf_attn_extend and tf_cache_append, where a chunk query's keys lie and which rows the append writes (tests/test_tf_extend_host.py,
# tests/test_gpu_tf_extend.py)
$(HARNESS_TF_EXTEND): tests/host_harness/harness_tf_extend.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the planner of option step_split: the partition of a token's visible keys over waves, blocks and lanes, the LDS bytes, both launches,
# the eligibility rule, where a key lies, the checks of flope_tf_stream_attention (tests/test_tf_step_split_host.py,
# tests/test_gpu_tf_step_split.py)
$(HARNESS_TF_SPLIT): tests/host_harness/harness_tf_split.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the planner of option extend_mfma: the eligibility rule, the key blocks and steps of tf_attn16_extend at unaligned first queries, where a
# key's LDS row comes from, the output rows, the launch, the checks of flope_tf_stream_attention_extend
# (tests/test_tf_extend_mfma_host.py, tests/test_gpu_tf_extend_mfma.py)
$(HARNESS_TF_EXTEND16): tests/host_harness/harness_tf_extend16.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the host side of a compiled attention mask: packing, the first / last tables, the validators, the per-length check, the pair counts,
# the masked launch (tests/test_tf_mask_host.py, tests/test_gpu_tf_mask.py); the test also builds the file as a stand-alone program
# under AddressSanitizer + UBSan (-DTF_MASK_MAIN) and runs it as a child process
$(HARNESS_TF_MASK): tests/host_harness/harness_tf_mask.cpp $(CSRC)/tf_attn_mask.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the tile map of a compiled mask for option mask_mfma: the per-query-block lists of key blocks, colany, the step classes, the corner
# prefix, the word and bit a lane reads, tf_attn_pick_masked and the launch of tf_attn_tiled_masked (tests/test_tf_mask16_host.py,
# tests/test_gpu_tf_mask16.py); the test also builds the file as a stand-alone program under AddressSanitizer + UBSan
# (-DTF_MASK16_MAIN) and runs it as a child process
$(HARNESS_TF_MASK16): tests/host_harness/harness_tf_mask16.cpp $(CSRC)/tf_attn_mask.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the host side of a compiled additive bias: the bit words derived from its -inf entries, the non-finite and plane-disagreement
# validators, the device layout, the index of an entry (tests/test_tf_bias_host.py, tests/test_gpu_tf_bias.py); the test also builds the
# file as a stand-alone program under AddressSanitizer + UBSan (-DTF_BIAS_MAIN) and runs it as a child process
$(HARNESS_TF_BIAS): tests/host_harness/harness_tf_bias.cpp $(CSRC)/tf_attn_mask.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# a stream state's distance table: the distances a state needs, the planes check, the first non-finite entry, the refusals of
# flope_tf_stream_open_bias, the entry a visible key reads, the keys <= D test of the biased kernels (tests/test_tf_stream_bias_host.py,
# tests/test_gpu_tf_stream_bias.py); the test also builds the file as a stand-alone program under AddressSanitizer + UBSan
# (-DTF_STREAM_BIAS_MAIN) and runs it as a child process
$(HARNESS_TF_STREAM_BIAS): tests/host_harness/harness_tf_stream_bias.cpp $(CSRC)/tf_encoder_stream.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# a compiled bias on the 16-bit MFMA attention (option bias_mfma): tf_attn_pick_biased, the device layout with the tile map behind the
# planes, the entry a lane of a taken step loads and the form of the load (tests/test_tf_bias16_host.py, tests/test_gpu_tf_bias16.py); the
# test also builds the file as a stand-alone program under AddressSanitizer + UBSan (-DTF_BIAS16_MAIN) and runs it as a child process
$(HARNESS_TF_BIAS16): tests/host_harness/harness_tf_bias16.cpp $(CSRC)/tf_attn_mask.h $(CSRC)/tf_attn_plan.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# conditioning figure and flag predicate of the guarded mode (tests/test_guard_host.py)
$(HARNESS_GUARD): tests/host_harness/harness_guard.cpp $(CSRC)/pose_math.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# strip plan of the depth statistics kernel: box extents, strip rows, tiled or untiled, the validity tile, the erosion element, the
# scratch layout (tests/depth_cases.py, tests/test_depth_cases.py, tests/test_gpu_depth_lift.py)
$(HARNESS_DEPTH): tests/host_harness/harness_depth.cpp $(CSRC)/depth_plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# tile plan of the crop + Lanczos-4 resize kernel: tile edge, LDS window, rows a tile touches, separable or direct path
# (tests/crop_cases.py, tests/test_crop_cases.py, tests/test_gpu_crop_cases.py)
$(HARNESS_CROP): tests/host_harness/harness_crop.cpp $(CSRC)/crop_plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the arithmetic of flope_frame_select: the count clamp and the per-row int16 cast, squarify and in-frame decision
# (tests/frame_cases.py, tests/test_frame_cases.py, tests/test_gpu_frame_cases.py)
$(HARNESS_FRAME): tests/host_harness/harness_frame.cpp $(CSRC)/frame_plan.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the device tracker's arithmetic (track_math.h, which track.hip's kernels call) and a scalar walk of a whole update with every
# index checked, with the broken copies the cases must notice (tests/track_cases.py, tests/test_track_host.py,
# tests/test_gpu_track.py); the test also builds the file as a stand-alone program under AddressSanitizer + UBSan (-DTRACK_MAIN)
# and runs it as a child process
$(HARNESS_TRACK): tests/host_harness/harness_track.cpp $(CSRC)/track_math.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the feed rule of a device-positioned stream state (tf_stream_feed.h, which tf_stream_feed_kernel calls per thread) in both row orders,
# with the broken copies the cases must notice, the token row, and track_math.h's track_measure for the expected token bits
# (tests/track_stream_cases.py, tests/test_tf_feed_host.py, tests/test_gpu_track_stream.py); the test also builds the file as a
# stand-alone program under AddressSanitizer + UBSan (-DTF_FEED_MAIN) and runs it as a child process
$(HARNESS_TF_FEED): tests/host_harness/harness_tf_feed.cpp $(CSRC)/tf_stream_feed.h $(CSRC)/track_math.h include/flope_amd.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the planner of option skinny (tf_skinny_plan.h, which tf_gemm_skinny calls per lane): the eligibility rule, the launch, and a walk of a
# whole launch that checks cover, bounds and that the fragments are the ones tf_gemm_mfma's LDS reads select (tests/test_tf_skinny_host.py,
# tests/test_gpu_tf_skinny.py); the test also builds the file as a stand-alone program under AddressSanitizer + UBSan (-DTF_SKINNY_MAIN)
# and runs it as a child process
$(HARNESS_TF_SKINNY): tests/host_harness/harness_tf_skinny.cpp $(CSRC)/tf_skinny_plan.h $(CSRC)/host_pack.h
	g++ -O2 -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the planner of option skinny_ln (tf_skinny_plan.h, which tf_gemm_skinny_ln calls per lane): the eligibility rule, the summation order of
# the statistics against tf_layernorm_vec's wave butterfly in float32 bit patterns (every product and sum rounded on its own: no
# contraction), and a walk of a whole launch that checks the store of the post-norm rows (tests/test_tf_skinny_ln_host.py,
# tests/test_gpu_tf_skinny_ln.py); the test also builds the file as a stand-alone program under AddressSanitizer + UBSan
# (-DTF_SKINNY_LN_MAIN) and runs it as a child process
$(HARNESS_TF_SKINNY_LN): tests/host_harness/harness_tf_skinny_ln.cpp $(CSRC)/tf_skinny_plan.h
	g++ -O2 -ffp-contract=off -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the encoder's architecture list (tf_arch_plan.h, which run_forward_with walks) against a brute-force statement of the post-norm and
# pre-norm orders, the skinny_ln fold rule, and tf_gelu_f32 (tf_act.h, which every linear kernel applies) measured against fp64 with every
# product and sum rounded on its own (tests/test_tf_arch_host.py, tests/test_gpu_tf_arch.py); the test also builds the file as a stand-alone
# program under AddressSanitizer + UBSan (-DTF_ARCH_MAIN) and runs it as a child process
$(HARNESS_TF_ARCH): tests/host_harness/harness_tf_arch.cpp $(CSRC)/tf_arch_plan.h $(CSRC)/tf_act.h
	g++ -O2 -ffp-contract=off -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<

# the same host code under AddressSanitizer + UBSan (sanitizers run on the CPU build only):
#   make asan-test      (builds the sanitized harness and runs tests/test_host.py against it; leak detection is off because the
#                        interpreter's own libcrypto allocations are reported as leaks at exit)
HARNESS_ASAN := tests/host_harness/libflope_host_harness_asan.so
$(HARNESS_ASAN): tests/host_harness/harness.cpp $(CSRC)/pose_math.h $(CSRC)/host_pack.h $(CSRC)/w4_sched.h $(CSRC)/plan.h
	g++ -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -fPIC -shared -std=c++17 -I$(CSRC) -o $@ $<
asan: $(HARNESS_ASAN)
asan-test: $(HARNESS_ASAN)
	ASAN_OPTIONS=detect_leaks=0 LD_PRELOAD=$$(gcc -print-file-name=libasan.so) FLOPE_HOST_HARNESS=$(HARNESS_ASAN) python -m pytest tests/test_host.py -q

# diagnostic build (ablation bits + in-kernel clock stamps of conv_stag; results of dbg options are wrong by construction):
#   make dbg && FLOPE_AMD_LIB=build/dbg/libflope_amd_dbg.so python tools/clock_probe.py
DBGDIR   := build/dbg
DBGOBJS  := $(patsubst $(CSRC)/%.hip,$(DBGDIR)/%.o,$(SRCS))
$(DBGDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(DBGDIR)
	$(HIPCC) $(HIPFLAGS) -DFLOPE_STAG_DBG -c $< -o $@
dbg: $(DBGOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(DBGDIR)/libflope_amd_dbg.so $(DBGOBJS)

clean:
	rm -rf build $(LIB) $(HARNESS) $(HARNESS_F32M) $(HARNESS_F32M_KSPLIT) $(HARNESS_GUARD) $(HARNESS_TF_F32M) $(HARNESS_TF_ATTN) $(HARNESS_TF_VARLEN) $(HARNESS_TF_FUSED) $(HARNESS_TF_CAUSAL) $(HARNESS_TF_STREAM) $(HARNESS_TF_WINDOW) $(HARNESS_TF_WINDOW16) $(HARNESS_TF_EXTEND) $(HARNESS_TF_SPLIT) $(HARNESS_TF_EXTEND16) $(HARNESS_TF_MASK) $(HARNESS_TF_MASK16) $(HARNESS_TF_BIAS) $(HARNESS_TF_STREAM_BIAS) $(HARNESS_TF_BIAS16) $(HARNESS_DEPTH) $(HARNESS_CROP) $(HARNESS_FRAME) $(HARNESS_TRACK) $(HARNESS_TF_FEED) $(HARNESS_TF_SKINNY) $(HARNESS_TF_SKINNY_LN) $(HARNESS_TF_ARCH)

# stand-alone measurement programs used by tools/collect_profiles.sh and DESIGN.md section 9 (not part of the library)
TOOLBINS := build/fetch_calib build/launch_floor build/loop_probe build/loop_probe32 build/dma_issue_probe
build/fetch_calib: tools/calib/fetch_calib.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
build/launch_floor: tools/calib/launch_floor.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
build/loop_probe: tools/probes/loop_probe.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
build/loop_probe32: tools/probes/loop_probe32.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
build/dma_issue_probe: tools/probes/dma_issue_probe.hip
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
tools: $(TOOLBINS)

.PHONY: all clean dbg tools asan asan-test
