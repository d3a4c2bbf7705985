# dict_rows.mk — builds dict_rows_test (make -f dict_rows.mk): the C++ mirror's DeviceDictionary and the Service over it, against
# ../../suggest_amd/libsuggest_hip.so, beside the Makefile's and mixed.mk's programs
ROCM ?= /opt/rocm
DROWS := _build/dict_rows_test
all: $(DROWS)
$(DROWS): dict_rows_test.cpp ../../include/suggest_hip.hpp ../../include/suggest_hip.h ../../suggest_amd/libsuggest_hip.so
	mkdir -p _build
	g++ -std=c++17 -O1 -Wall -pthread dict_rows_test.cpp -o $(DROWS) -L../../suggest_amd -lsuggest_hip \
	    -Wl,-rpath,'$$ORIGIN/../../../suggest_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath-link,$(ROCM)/lib
clean-dict-rows:
	rm -f $(DROWS)
