# edit_search.mk — builds edit_search_test (make -f edit_search.mk): the C++ mirror's DeviceDictionary::EditSearch, against
# ../../suggest_amd/libsuggest_hip.so, beside the Makefile's, mixed.mk's, dict_rows.mk's and edit_rank.mk's programs
ROCM ?= /opt/rocm
ESEARCH := _build/edit_search_test
all: $(ESEARCH)
$(ESEARCH): edit_search_test.cpp ../../include/suggest_hip.hpp ../../include/suggest_hip.h ../../suggest_amd/libsuggest_hip.so
	mkdir -p _build
	g++ -std=c++17 -O1 -Wall -pthread edit_search_test.cpp -o $(ESEARCH) -L../../suggest_amd -lsuggest_hip \
	    -Wl,-rpath,'$$ORIGIN/../../../suggest_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath-link,$(ROCM)/lib
clean-edit-search:
	rm -f $(ESEARCH)
