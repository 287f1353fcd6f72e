# The host driver of witness digest v2 (tests/test_fs_stream_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.
#   make -f fs_stream.mk fs_stream_host fs_stream_host_san
include Makefile
FDEPS = fs_stream_host.cpp $(CSRC)/witness_tree.hpp $(CSRC)/fs.hpp $(CSRC)/sha256.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
fs_stream_host: $(FDEPS)
	$(CXX) -O2 -std=c++17 -w fs_stream_host.cpp -o $@
fs_stream_host_san: $(FDEPS)
	$(CXX) $(SAN) fs_stream_host.cpp -o $@
