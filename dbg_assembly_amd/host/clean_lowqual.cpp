// clean_lowqual -- the clean_illumina module's low-quality trimmer (clean_illumina/clean_lowqual.cpp) with the error sums and the
// block search made on the GPU (CLEAN section of include/dbgk.h).  Same command line, same two output files: the trimmed reads
// (gzip) and the statistics.  -t sizes nothing on the device.
#include "clean_common.h"

static double Error_rate_cutoff = 0.001;
static int Min_read_len = 75;
static int Quality_shift = 33;
static int threadNum = 3;

static void usage()
{
	cout << "Description:\nclean_lowqual detects and trims the low quality parts in a reads, and output a largest block in which the average "
	        "error rate is lower than a given cutoff(-e). The programs gets all the blocks in a reads with average error rate lower than the "
	        "cutoff (-e), and choose the longest block as the final result (trimmed reads).   The illumina sequencing machine produces reads "
	        "with average error rate of 1%, however, the error bases are not distributed evenly. By set a cutoff (-e) of 0.1% for the average "
	        "error rate, we can exclude most of(90%) of the sequencing errors by filtering out only a small ratio read sequences. The program "
	        "also has a function to filter the extreme short reads by using a cutoff (-r); The program runs in a multiple thread mode (-t). "
	        "The input file should be fastq or gzipped-fasts format, and there are two result files: one is the high-quality reads file, and "
	        "the other one is a statistics file.\n";
	cout << "\nUsage:\n  clean_lowqual <input.fq.gz>  <output.fq.gz>  <output.stat>" << endl;
	cout << "   Author: Fanwei, fanweiagis@126.com" << endl;
	cout << "   Version 1.0;" << endl;
	cout << "   -e <float>  average error rate cutoff for a read, default=" << Error_rate_cutoff << endl;
	cout << "   -q <int>    base quality shift value, default=" << Quality_shift << endl;
	cout << "   -r <int>    minimum read length for output, default=" << Min_read_len << endl;
	cout << "   -t <int>    thread number to run in parallel, default=" << threadNum << endl;
	cout << "   -h          get help information" << endl << endl;
	cout << "Example:\n  ../clean_lowqual -e 0.001 -r 75 sequencing_data_R1.fq.gz sequencing_data_R1.fq.gz.nonLowQual.gz "
	        "sequencing_data_R1.fq.gz.nonLowQual.stat\n" << endl;
	exit(0);
}

// what the program appends to a record's header (clean_lowqual.cpp:79-183): seq_len is the read's length after a record whose two
// strings differ in length was emptied, is_short says that what is left of it is shorter than -r.  Both routes call it.
static void lowqual_suffix(const dbgk_lowqual_block &b, int seq_len, bool is_short, string &out)
{
	char number[64];
	// boost::lexical_cast<std::string>(double) writes 17 significant digits
	snprintf(number, sizeof number, "%.17g", b.error_sum / seq_len * 100);
	out += "    RQ: ";
	out += number;
	out += "%";
	if (b.trimmed) out += "  TrimLowQual";
	if (is_short) out += "  FilterShort";
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "e:r:q:t:h")) != -1) {
		switch (c) {
			case 'e': Error_rate_cutoff = atof(optarg); break;
			case 'r': Min_read_len = atoi(optarg); break;
			case 'q': Quality_shift = atoi(optarg); break;
			case 't': threadNum = atoi(optarg); break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 4 || argc - optind < 3) usage();
	if (Quality_shift < 0 || Quality_shift > 127) {
		cerr << "the base quality shift (-q) must lie in 0..127" << endl;
		return 1;
	}
	const string in_reads1_file = argv[optind++];
	const string out_reads1_file = argv[optind++];
	const string out_stat_file = argv[optind++];
	const clock_t time_start = clock();
	cerr << "\nProgram starting\n";

	dbgk_clean *cleaner = nullptr;
	int rc = dbgk_clean_create(0, &cleaner);
	if (rc) die("dbgk_clean_create", rc);

	uint64_t total_raw_reads = 0, total_raw_bases = 0, total_filtered_lowqual_reads = 0, total_filtered_lowqual_bases = 0;
	uint64_t total_filtered_short_reads = 0, total_filtered_short_bases = 0, total_clean_reads = 0, total_clean_bases = 0;
	if (text_on_device()) {
		GzWriter cleanfile1(out_reads1_file);
		DeviceTextTotals T;
		vector<dbgk_lowqual_block> blocks;
		clean_text_on_device(in_reads1_file, cleanfile1, cleaner, Min_read_len, false, T,
		                     [&](const char *d_bases, const char *d_quals, const uint64_t *offsets, const uint64_t *lens, uint64_t n, string &suffix,
		                         vector<uint64_t> &suffix_offsets) {
			blocks.resize(n + 1);
			const int rc = dbgk_clean_lowqual_device(cleaner, d_bases, d_quals, offsets, n, Error_rate_cutoff, Quality_shift, blocks.data());
			if (rc) die("dbgk_clean_lowqual_device", rc);
			for (uint64_t i = 0; i < n; i++) {
				const dbgk_lowqual_block &b = blocks[i];
				const uint64_t kept = b.trimmed ? (b.start >= 1 ? (uint64_t)b.length : 0) : lens[i];
				lowqual_suffix(b, (int)lens[i], kept < (uint64_t)Min_read_len, suffix);
				suffix_offsets.push_back(suffix.size());
			}
		});
		cleanfile1.close();
		total_raw_reads = T.raw_reads, total_raw_bases = T.raw_bases;
		total_filtered_lowqual_reads = T.trimmed_reads, total_filtered_lowqual_bases = T.trimmed_bases;
		total_filtered_short_reads = T.short_reads, total_filtered_short_bases = T.short_bases;
		total_clean_reads = T.clean_reads, total_clean_bases = T.clean_bases;
	} else {
		LineReader infile1(in_reads1_file);
		GzWriter cleanfile1(out_reads1_file);
		RecordBatch batch;
		vector<dbgk_lowqual_block> blocks;
		string bases, quals;
		vector<uint64_t> offsets;
		for (bool more = true; more;) {
			more = batch.fill(infile1, total_raw_reads, total_raw_bases);
			cerr << "reading num " << batch.size() << endl;
			for (size_t i = 0; i < batch.size(); i++) // a record whose two strings differ in length is emptied (clean_lowqual.cpp:74-77)
				if (batch.reads[i].size() != batch.quals[i].size()) {
					batch.reads[i] = "";
					batch.quals[i] = "";
				}
			concat(batch.reads, bases, offsets);
			concat(batch.quals, quals, offsets);
			blocks.resize(batch.size() + 1);
			rc = dbgk_clean_lowqual(cleaner, bases.data(), quals.data(), offsets.data(), batch.size(), Error_rate_cutoff, Quality_shift, blocks.data());
			if (rc) die("dbgk_clean_lowqual", rc);
			for (size_t i = 0; i < batch.size(); i++) { // thread_cleanlowqual (clean_lowqual.cpp:79-183)
				const dbgk_lowqual_block &b = blocks[i];
				string &read = batch.reads[i], &qual = batch.quals[i];
				const int seq_len = (int)read.size();
				for (int j = 0; j < seq_len; j++)
					if (read[j] == 'N') qual[j] = (char)Quality_shift;
				if (b.trimmed) {
					if (b.start >= 1) {
						read = read.substr(b.start - 1, b.length);
						qual = qual.substr(b.start - 1, b.length);
					} else {
						read = "";
						qual = "";
					}
					total_filtered_lowqual_reads++;
					total_filtered_lowqual_bases += seq_len - b.length;
				}
				const bool is_short = read.size() < (size_t)Min_read_len;
				lowqual_suffix(b, seq_len, is_short, batch.heads[i]);
				if (is_short) {
					total_filtered_short_reads++;
					total_filtered_short_bases += read.size();
					read = "";
					qual = "";
				}
				if (read.size()) {
					total_clean_reads++;
					total_clean_bases += read.size();
				}
			}
			batch.write(cleanfile1);
			batch.clear();
		}
		cleanfile1.close();
	}
	dbgk_clean_destroy(cleaner);

	ofstream statfile(out_stat_file.c_str());
	statfile << "#total_raw_reads:   " << total_raw_reads << endl;
	statfile << "#total_raw_bases:   " << total_raw_bases << endl;
	statfile << "#filtered_lowqual_reads: " << total_filtered_lowqual_reads << "\t" << (double)total_filtered_lowqual_reads / total_raw_reads * 100 << "%" << endl;
	statfile << "#filtered_lowqual_bases: " << total_filtered_lowqual_bases << "\t" << (double)total_filtered_lowqual_bases / total_raw_bases * 100 << "%" << endl;
	statfile << "#filtered_short_reads: " << total_filtered_short_reads << "\t" << (double)total_filtered_short_reads / total_raw_reads * 100 << "%" << endl;
	statfile << "#filtered_short_bases: " << total_filtered_short_bases << "\t" << (double)total_filtered_short_bases / total_raw_bases * 100 << "%" << endl;
	statfile << "#total_clean_reads: " << total_clean_reads << "\t" << total_clean_reads / (double)total_raw_reads * 100 << "%" << endl;
	statfile << "#total_clean_bases: " << total_clean_bases << "\t" << total_clean_bases / (double)total_raw_bases * 100 << "%" << endl;

	cerr << "\nAll jobs finishd done\n";
	cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl;
	return 0;
}
