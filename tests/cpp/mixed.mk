# mixed.mk — builds the mixed batch's C++ programs (make -f mixed.mk) against ../../suggest_amd/libsuggest_hip.so, beside the Makefile's:
# suggest_many_test (the C++ mirror's SuggestMany) and mixed_load (single-query callers over several keys; tools/mixed_timing.py)
ROCM ?= /opt/rocm
MANY := _build/suggest_many_test
MLOAD := _build/mixed_load
all: $(MANY) $(MLOAD)
$(MANY): suggest_many_test.cpp ../../include/suggest_hip.hpp ../../include/suggest_hip.h ../../suggest_amd/libsuggest_hip.so
	mkdir -p _build
	g++ -std=c++17 -O1 -Wall -pthread suggest_many_test.cpp -o $(MANY) -L../../suggest_amd -lsuggest_hip \
	    -Wl,-rpath,'$$ORIGIN/../../../suggest_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath-link,$(ROCM)/lib
$(MLOAD): mixed_load.cpp ../../include/suggest_hip.h ../../suggest_amd/libsuggest_hip.so
	mkdir -p _build
	g++ -std=c++17 -O2 -Wall -pthread mixed_load.cpp -o $(MLOAD) -L../../suggest_amd -lsuggest_hip \
	    -Wl,-rpath,'$$ORIGIN/../../../suggest_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath-link,$(ROCM)/lib
clean-mixed:
	rm -f $(MANY) $(MLOAD)
