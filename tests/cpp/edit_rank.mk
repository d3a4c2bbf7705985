# edit_rank.mk — builds edit_rank_test (make -f edit_rank.mk): the C++ mirror's EditDistances and SuggestEdit, against
# ../../suggest_amd/libsuggest_hip.so, beside the Makefile's, mixed.mk's and dict_rows.mk's programs
ROCM ?= /opt/rocm
ERANK := _build/edit_rank_test
all: $(ERANK)
$(ERANK): edit_rank_test.cpp ../../include/suggest_hip.hpp ../../include/suggest_hip.h ../../suggest_amd/libsuggest_hip.so
	mkdir -p _build
	g++ -std=c++17 -O1 -Wall -pthread edit_rank_test.cpp -o $(ERANK) -L../../suggest_amd -lsuggest_hip \
	    -Wl,-rpath,'$$ORIGIN/../../../suggest_amd' -Wl,-rpath,$(ROCM)/lib -Wl,-rpath-link,$(ROCM)/lib
clean-edit-rank:
	rm -f $(ERANK)
