# Build of the eMI355X backend (no cmake/ninja needed; hipcc + g++ + make).
#
#   make            -> etol_amd/lib/libemi355x.so      (HIP kernels + C ABI, gfx950)
#                      etol_amd/lib/libetol_mi355x.so  (C++ host: TrajectoryOptimizer + eMI355X)
#                      etol_amd/lib/etol_mi355x_example1, tests/harness/libetol_harness.so
#   make oracle     -> oracle/liboracle.so, oracle/libepsopt_style.so  (test infrastructure)
#
# Built artefacts are git-ignored but travel to the GPU box with the snapshot.
ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
CXX       ?= g++
CC        ?= gcc
ARCH      ?= gfx950
LIBDIR    := etol_amd/lib
CSRC      := etol_amd/csrc
HOST      := etol_amd/host

HIPFLAGS  := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-function -Wno-inline-asm $(EXTRA_HIPFLAGS)
CXXFLAGS  := -O2 -std=c++17 -fPIC -Iinclude -Wall
XML2_INC  := -I/usr/include/libxml2
XML2_LIB  := -lxml2

.PHONY: all lib host oracle clean check-keep-record check-refine-book check-restart-book check-nlp check-mesh-driver check-ode-operator check-ode-delay-operator check-plan-route check-pass-plan check-param-table-plan check-pass-registers check-pass-residency check-pass-work
ifneq ($(wildcard etol_amd/host/eMI355X.cpp),)
all: lib host oracle
else
all: lib oracle
endif

lib: $(LIBDIR)/libemi355x.so
host: $(LIBDIR)/libetol_mi355x.so $(LIBDIR)/etol_mi355x_example1 $(LIBDIR)/etol_mi355x_montecarlo tests/harness/libetol_harness.so

$(LIBDIR):
	mkdir -p $(LIBDIR)

CSRC_HDR  := $(wildcard $(CSRC)/*.hpp) include/emi355x.h
# headers a model program compiled at run time (hiprtc, emi_rtc.hip) includes: embedded as text
RTC_HDR   := $(CSRC)/emi_models.hpp $(CSRC)/emi_pass_work.hpp $(CSRC)/emi_args.hpp $(CSRC)/emi_node_kernels.hpp $(CSRC)/emi_symdefect_kernels.hpp

$(LIBDIR)/%.o: $(CSRC)/%.hip $(CSRC_HDR) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(LIBDIR)/emi_rtc_sources.inc: $(RTC_HDR) tools/embed_src.py | $(LIBDIR)
	python3 tools/embed_src.py $@ $(RTC_HDR)
$(LIBDIR)/emi_rtc.o: $(CSRC)/emi_rtc.hip $(LIBDIR)/emi_rtc_sources.inc $(CSRC_HDR) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -I$(LIBDIR) -c $< -o $@
# -ffp-contract=off: emi_plan_route's bits are single rounded operations (emi_plan_route.hpp), whatever the target has
$(LIBDIR)/emi_host.o: $(CSRC)/emi_host.cpp $(CSRC)/emi_plan_route.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(CXXFLAGS) -ffp-contract=off -c $< -o $@
# RCCL gather (librccl is dlopen'ed at first use, not linked)
$(LIBDIR)/emi_comm.o: $(CSRC)/emi_comm.cpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -c $< -o $@

LIB_OBJ := emi_kernels emi_kernels_tab emi_symdefect emi_defect_f32 emi_api emi_api_pass emi_api_adjoint emi_api_kkt emi_api_ipm emi_api_ode emi_rtc emi_kkt emi_adjoint \
           emi_kkt_blocks emi_ipm emi_ipm_solve emi_ipm_ladder emi_ode_error emi_start_guess emi_api_start emi_host emi_comm
$(LIBDIR)/libemi355x.so: $(LIB_OBJ:%=$(LIBDIR)/%.o)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -L$(ROCM)/lib -lhiprtc -lrocsolver -lrocblas -ldl

HOST_SRC := $(HOST)/TrajectoryOptimizer.cpp $(HOST)/eMI355X.cpp $(HOST)/emi_nlp.cpp $(HOST)/emi_mesh_driver.cpp $(HOST)/emi_trace.cpp
HOST_HDR := $(wildcard include/ETOL/*.hpp) $(wildcard $(HOST)/*.hpp) include/emi355x.h

# the host side of the Newton step (block eigen-decompositions, r x r Cholesky of the low-rank correction) wants AVX2
$(LIBDIR)/libetol_mi355x.so: CXXFLAGS := -O3 -march=x86-64-v3 -fopenmp-simd -std=c++17 -fPIC -Iinclude -Wall
$(LIBDIR)/libetol_mi355x.so: $(HOST_SRC) $(HOST_HDR) $(LIBDIR)/libemi355x.so
	$(CXX) $(CXXFLAGS) $(XML2_INC) -I$(HOST) -shared -o $@ $(HOST_SRC) -L$(LIBDIR) -lemi355x $(XML2_LIB) \
		-Wl,-rpath,'$$ORIGIN'

$(LIBDIR)/etol_mi355x_example1: etol_amd/examples/etol_mi355x_example1.cpp $(LIBDIR)/libetol_mi355x.so
	$(CXX) $(CXXFLAGS) -I$(HOST) -o $@ $< -L$(LIBDIR) -letol_mi355x -lemi355x -Wl,-rpath,'$$ORIGIN'

$(LIBDIR)/etol_mi355x_montecarlo: etol_amd/examples/etol_mi355x_montecarlo.cpp $(LIBDIR)/libetol_mi355x.so
	$(CXX) $(CXXFLAGS) -I$(HOST) -pthread -o $@ $< -L$(LIBDIR) -letol_mi355x -lemi355x -Wl,-rpath,'$$ORIGIN'

HARNESS_SRC := tests/harness/etol_harness.cpp tests/harness/etol_harness_certify.cpp tests/harness/etol_harness_delay_certify.cpp tests/harness/etol_harness_blocks.cpp tests/harness/etol_harness_ipm.cpp tests/harness/etol_harness_lockstep.cpp tests/harness/etol_harness_ladder.cpp tests/harness/etol_harness_rescue.cpp \
               tests/harness/etol_harness_ode_error.cpp tests/harness/etol_harness_track_ladder.cpp tests/harness/etol_harness_delay_ode_error.cpp \
               tests/harness/etol_harness_param_table.cpp
tests/harness/libetol_harness.so: $(HARNESS_SRC) $(LIBDIR)/libetol_mi355x.so $(HOST_HDR) $(CSRC)/emi_ipm_control.hpp
	$(CXX) $(CXXFLAGS) -I$(HOST) -I$(CSRC) -shared -o $@ $(HARNESS_SRC) -L$(LIBDIR) -letol_mi355x -lemi355x -ldl \
		-Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

oracle:
	$(MAKE) -C oracle

# the bookkeeping behind EMI_EVAL_KEEP_INVARIANT (emi_keep_record.hpp, host-only) as a stand-alone program under the host sanitizers
KEEP_CHECK_OUT ?= $(LIBDIR)/keep_record_check
check-keep-record: tests/harness/keep_record_main.cpp $(CSRC)/emi_keep_record.hpp | $(LIBDIR)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -I$(CSRC) -o $(KEEP_CHECK_OUT) $<
	$(KEEP_CHECK_OUT)

# the bookkeeping of the lock-step ladder and refinement (emi_refine_book.hpp, host-only: who is live, who retires where) as a
# stand-alone program under the host sanitizers, with scripted statuses and estimates; the rule comes from emi_host.cpp
BOOK_CHECK_OUT ?= $(LIBDIR)/refine_book_check
check-refine-book: tests/harness/refine_book_main.cpp $(CSRC)/emi_refine_book.hpp $(CSRC)/emi_host.cpp include/emi355x.h | $(LIBDIR)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Iinclude -I$(CSRC) -o $(BOOK_CHECK_OUT) \
		tests/harness/refine_book_main.cpp $(CSRC)/emi_host.cpp -lm
	$(BOOK_CHECK_OUT)

# the bookkeeping of the ladder restarts (emi_restart_book.hpp over emi_refine_book.hpp, host-only: who is pending, which attempt owns
# an instance's output, the drop rule) as a stand-alone program under the host sanitizers, with scripted statuses and estimates
RESTART_CHECK_OUT ?= $(LIBDIR)/restart_book_check
check-restart-book: tests/harness/restart_book_main.cpp $(CSRC)/emi_restart_book.hpp $(CSRC)/emi_refine_book.hpp $(CSRC)/emi_host.cpp include/emi355x.h | $(LIBDIR)
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Iinclude -I$(CSRC) -o $(RESTART_CHECK_OUT) \
		tests/harness/restart_book_main.cpp $(CSRC)/emi_host.cpp -lm
	$(RESTART_CHECK_OUT)

# the NLP iteration (emi_nlp.cpp: its state object, the steps and iterates it copies and takes back) as a stand-alone program under
# the host sanitizers, on the CPU oracle: no Python, no device
SANITIZE      := -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
NLP_CHECK_OUT ?= $(LIBDIR)/nlp_sanitize_check
check-nlp: tests/harness/nlp_sanitize_main.cpp $(HOST)/emi_nlp.cpp $(HOST)/emi_nlp.hpp $(CSRC)/emi_host.cpp oracle/emi_oracle.c | $(LIBDIR)
	$(CC) $(SANITIZE) -std=c99 -c oracle/emi_oracle.c -o $(NLP_CHECK_OUT)_oracle.o
	$(CXX) $(SANITIZE) -std=c++17 -Iinclude -I$(HOST) -o $(NLP_CHECK_OUT) tests/harness/nlp_sanitize_main.cpp $(HOST)/emi_nlp.cpp $(CSRC)/emi_host.cpp \
		$(NLP_CHECK_OUT)_oracle.o -lm
	$(NLP_CHECK_OUT)

# the mesh strategy of solve() (emi_mesh_driver.cpp: ladder, restarts, retries, budget, refinement) as a stand-alone program under the
# host sanitizers, with a scripted solver behind its host interface: no Python, no device (the device library is linked for the
# symbols of eMI355X.cpp, whose guess builders the strategy calls; none of them is called).  -O0: the program decides, it does not compute
MESH_CHECK_OUT ?= $(LIBDIR)/mesh_driver_check
MESH_CHECK_SRC := tests/harness/mesh_driver_main.cpp $(HOST_SRC) $(CSRC)/emi_host.cpp
$(MESH_CHECK_OUT)_obj/%.o: %.cpp $(HOST_HDR)
	@mkdir -p $(dir $@)
	$(CXX) $(SANITIZE:-O1=-O0) -std=c++17 -Iinclude -I$(HOST) $(XML2_INC) -c $< -o $@
check-mesh-driver: $(MESH_CHECK_SRC:%.cpp=$(MESH_CHECK_OUT)_obj/%.o) $(LIBDIR)/libemi355x.so
	$(CXX) $(SANITIZE) -o $(MESH_CHECK_OUT) $(filter %.o,$^) -L$(LIBDIR) -lemi355x $(XML2_LIB) -lm -Wl,-rpath,$(abspath $(LIBDIR))
	$(MESH_CHECK_OUT)

# the operator builder of the ODE-error call (emi_ode_error_operator, csrc/emi_host.cpp: host-only) as a stand-alone program under the
# host sanitizers
ODE_OP_CHECK_OUT ?= $(LIBDIR)/ode_operator_check
check-ode-operator: tests/harness/ode_operator_main.cpp $(CSRC)/emi_host.cpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -std=c++17 -Iinclude -o $(ODE_OP_CHECK_OUT) tests/harness/ode_operator_main.cpp $(CSRC)/emi_host.cpp -lm
	$(ODE_OP_CHECK_OUT)

# the operator of one delay between the nodes (emi_ode_error_delay_operator, csrc/emi_host.cpp: host-only), the same way
ODE_DEL_CHECK_OUT ?= $(LIBDIR)/ode_delay_operator_check
check-ode-delay-operator: tests/harness/ode_delay_operator_main.cpp $(CSRC)/emi_host.cpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -ffp-contract=off -std=c++17 -Iinclude -o $(ODE_DEL_CHECK_OUT) tests/harness/ode_delay_operator_main.cpp $(CSRC)/emi_host.cpp -lm
	$(ODE_DEL_CHECK_OUT)

# the planned route (emi_plan_route, csrc/emi_host.cpp with csrc/emi_plan_route.hpp: host-only) on the fixtures of tests/golden as a
# stand-alone program under the host sanitizers
PLAN_CHECK_OUT ?= $(LIBDIR)/plan_route_check
check-plan-route: tests/harness/plan_route_main.cpp $(CSRC)/emi_host.cpp $(CSRC)/emi_plan_route.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -ffp-contract=off -std=c++17 -Iinclude -o $(PLAN_CHECK_OUT) tests/harness/plan_route_main.cpp $(CSRC)/emi_host.cpp -lm
	$(PLAN_CHECK_OUT) tests/golden/plan_cases.json

# the launch policy of the fp64 evaluation pass (emi_pass_plan.hpp, host-only: form table, bands, resolve_form, plan_pass, plan_piece) as a
# stand-alone program under the host sanitizers, over the grid of tools/api_identity.py plan
PASS_PLAN_CHECK_OUT ?= $(LIBDIR)/pass_plan_check
check-pass-plan: tests/harness/pass_plan_main.cpp $(CSRC)/emi_pass_plan.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -std=c++17 -Wall -Iinclude -I$(CSRC) -o $(PASS_PLAN_CHECK_OUT) tests/harness/pass_plan_main.cpp
	$(PASS_PLAN_CHECK_OUT)

# ... and what that policy makes of a context with a per-instance parameter table (PassPolicyIn::param_table: never overlapped, never one
# launch, no pieces, the report of "overlap" 0), the same way
PARAM_PLAN_CHECK_OUT ?= $(LIBDIR)/param_table_plan_check
check-param-table-plan: tests/harness/param_table_plan_main.cpp $(CSRC)/emi_pass_plan.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -std=c++17 -Wall -Iinclude -I$(CSRC) -o $(PARAM_PLAN_CHECK_OUT) tests/harness/param_table_plan_main.cpp
	$(PARAM_PLAN_CHECK_OUT)

# the residency rule of that policy ("sym_res": three resident workgroups per CU only with a direct-operator row, the default by band, built-in
# models only, the order in which resolve_form grants the wants) as a stand-alone program under the host sanitizers
PASS_RES_CHECK_OUT ?= $(LIBDIR)/pass_residency_check
check-pass-residency: tests/harness/pass_residency_main.cpp $(CSRC)/emi_pass_plan.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -std=c++17 -Wall -Iinclude -I$(CSRC) -o $(PASS_RES_CHECK_OUT) tests/harness/pass_residency_main.cpp
	$(PASS_RES_CHECK_OUT)

# the work table of the one-launch pass (emi_pass_work.hpp, host-only builder over pass_role_of and ring_tile_of; its key from the plan,
# emi_pass_plan.hpp) as a stand-alone program under the host sanitizers: every entry against the two maps, every (tile, slice) and every
# node chunk exactly once, every other block idle, over models, meshes, batches, block orders, tile orders, K slices and K halves
PASS_WORK_CHECK_OUT ?= $(LIBDIR)/pass_work_check
check-pass-work: tests/harness/pass_work_main.cpp $(CSRC)/emi_pass_work.hpp $(CSRC)/emi_pass_plan.hpp include/emi355x.h | $(LIBDIR)
	$(CXX) $(SANITIZE) -std=c++17 -Wall -Iinclude -I$(CSRC) -o $(PASS_WORK_CHECK_OUT) tests/harness/pass_work_main.cpp
	$(PASS_WORK_CHECK_OUT)

# the register budget of emi_pass_f64_kernel: every instantiation compiled for $(ARCH) (device code only, nothing is kept) and held to the
# resident workgroups per CU it states -- 3: occupancy 3, at most 168 registers, no scratch; 2: no scratch and what tools/pass_registers.json
# records.  No device needed.
check-pass-registers: tools/check_pass_registers.py tools/pass_registers.json $(CSRC)/emi_symdefect.hip $(CSRC_HDR)
	python3 tools/check_pass_registers.py --hipcc $(HIPCC) --arch $(ARCH)

clean:
	rm -rf $(LIBDIR) tests/harness/*.so
	$(MAKE) -C oracle clean
